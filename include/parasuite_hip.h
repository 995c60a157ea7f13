/*
 * parasuite_hip.h -- C ABI of libparasuite_hip.so, the MI355X (gfx950) replacement for the
 * aligner child processes of PARA-suite's `map` command.
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   ps_index        <- exec `bwa index <ref>`                     src/src/mapping/PARAsuiteMapping.java:45-55,
 *                                                                 src/src/mapping/BWAMapping.java:35-45
 *   ps_map          <- exec `bwa parasuite -t T -X mm -p EP -g IP ref fq -f P.sai`
 *                      + `bwa samse ref P.sai fq -f P.sam`        PARAsuiteMapping.java:63-77,84-92
 *                      (error_profile == NULL: `bwa aln -t T -n mm` + samse,  BWAMapping.java:51-61,68-75)
 *   ps_last_error   <- child exit status + inherited stderr       src/src/mapping/Mapping.java:151-198
 * The Java method these sit behind is Mapping.executeMapping(int threads, String reference,
 * String input, String outputPrefix, int mappingQualityFilter, String additionalOptions)
 * (Mapping.java:40-42); INTEGRATION.md shows the JNI subclass and the argv-compatible `bwa` shim.
 *
 * Conventions: UTF-8 paths, int return 0 = success / non-zero = failure (message via
 * ps_last_error() and on stderr), synchronous, one call at a time per process, never exit()s or
 * throws across the boundary.  There is no CPU implementation: without a HIP device every
 * computing entry point fails.
 */
#ifndef PARASUITE_HIP_H
#define PARASUITE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char *ps_version(void);
const char *ps_last_error(void);

/* `bwa index`: writes <ref_fa>.bwt/.sa/.pac/.ann (this project's formats; the caller only tests that
 * <ref_fa>.bwt exists, PARAsuiteMapping.java:45-46).  Suffix sorting runs on the GPU.
 * ref_fa: FASTA as plain text, gzip (RFC 1952, concatenated members too) or BGZF, told apart by its first two bytes, as bwa
 * reads it through gzopen.  The index files are named after the path as given (genome.fa.gz.bwt, ...), as `bwa index` names
 * them; every call that takes ref_fa takes the same string.  Deviations: as for the reads of ps_map.
 * Output files on failure, for this call and every call below that writes files: outputs
 * are written under <name>.<mode>-tmp and renamed when complete; on error no output of the call exists under its final or its
 * temporary name, a file from before the call is either untouched or fully replaced, and an output that is one of the call's
 * inputs is refused.  Not so the streamed SAM / BAM of ps_map, ps_map_opts, ps_map_profiled and ps_map_to_bam: written in place. */
int ps_index(const char *ref_fa);

/* `bwa parasuite` (or `bwa aln` when error_profile is NULL) + `bwa samse` fused: FASTQ in, SAM out.
 * threads: host worker threads for parsing/formatting (the reference's -t).  mm: the -X (profile
 * mode) or -n (stock mode) argument as the Java passes it, e.g. "-1", "2", "0.04".
 * Devices: the first PARASUITE_GPUS (environment, default 1), each with its own copy of the index; the
 * input is cut into pieces that a parser thread, the device workers and a SAM writer work on side by
 * side; the output does not depend on the cut or on the number of devices.
 * Accepted ranges (here and for ps_ctx_set_*; what lies outside is an error naming the limit, never a launch):
 *   profile -X x: 0..15 (a budget of 8x units: 8x + 1 score buckets, at most PS_MAX_BUCKETS = 128; -X 16 is refused).
 *     -X -1: BWA's per-length budget cal_maxdiff(len, 0.02, 0.04): 7 differences up to 189 bp, 8 from 190, 9 at 225-250.
 *   stock -n INT: 0..37 (3n + 15 score buckets; -n 38 is refused); -n with a '.' is a false-negative rate.
 *   read length: 1..250 bp (PS_MAX_LEN); one longer read fails the call.
 * Above 64 score buckets (-X 8 and up, -X -1 from 190 bp, -n 17 and up) a launch takes the wide search stack; reads with the
 * same gap limit share one launch, which the longest of them decides.
 * fastq: FASTQ or FASTA as plain text, gzip (RFC 1952: CM 8, FEXTRA / FNAME / FCOMMENT / FHCRC skipped, CRC32 and ISIZE of
 * every member checked, concatenated members decoded one after the other) or BGZF, a regular file or a FIFO, told apart by the
 * first two bytes -- what bwa accepts through gzopen.  gzip is inflated by one thread that runs ahead of the parser, BGZF block
 * by block on `threads`; the text's size is unknown then, so the pieces are cut as for a FIFO (csrc/ps_inflate.h).  The same
 * holds for ps_map_to_bam, ps_map_profiled, ps_map_route's reads and ps_batch_from_fastq.
 * Deviations: (1) gzread hands out a truncated stream as if it ended there, so bwa maps half a file and exits 0; here an input
 * that ends inside a member (header, data or trailer) fails the call.  (2) gzread ignores bytes behind the last member; here
 * bytes behind a complete member that do not start another member fail the call.  Both, a CRC32 / ISIZE mismatch, invalid
 * deflate data, CM other than 8, reserved flag bits and a bad BGZF BSIZE are errors that name the file and the compressed byte.
 * (3) A FASTQ text that was cut off behind the '+' line of its last record ("@name", one line of bases, "+..." and the end: bases
 * and no quality line) fails the call and names the file and the read; kseq drops such a record without a word. */
int ps_map(int threads, const char *mm, const char *error_profile, const char *indel_profile,
           const char *ref_fa, const char *fastq, const char *out_sam);

/* ---- the search options of `bwa aln` and `bwa samse` beyond -n / -X ----------------------------------------------------------
 * Defaults are upstream's (BWA 0.7.x gap_opt_t; samse -n 3): with them, or with NULL, every call computes what it computed before
 * these options existed.  A value is accepted where the result is exactly upstream's rule; anything else is refused before any
 * launch with the field and its limit in ps_last_error() -- never clamped into a different result:
 *   max_gap_opens       0..7   the narrow stack entry counts opens in 3 bits, and 2*7 + 1 CIGAR operations fit a ps_hit; -o 8 is refused
 *   max_gap_extensions  ..15   the launch header's 4 bits; -e 16 is refused.  Every value below 1 is the k-difference mode
 *   indel_end_skip      0..    255 and up mean "no gap anywhere": no read is longer than 250 bp
 *   max_del_occ         0..255
 *   seed_len            1..    from the read length on: no seed
 *   max_seed_diff       0..4095 (stock), 0..511 (profile costs count a difference as 8 units; 12 bits of units in the launch header)
 *   max_entries         1..2000000   what the largest search tier holds, and upstream's default
 *   s_mm, s_gapo, s_gape  0..255 each; together with -n they also decide the number of score buckets, at most PS_MAX_BUCKETS = 128:
 *                       a table past that fails at ps_batch_from_fastq / ps_batch_from_codes / ps_map_opts, as a -n out of range does
 *   max_top2            0..    255 and up take the wide search stack
 *   max_alt_hits        0..    0: no XA tag
 * A launch whose gap limits add up to more than 7 (-o 2 and up in the k-difference mode, -e 7 and up) takes the wide search stack,
 * whose entries count in bytes.  A gapped hit whose CIGAR comes out of the banded alignment with more than 16 operations fails the
 * call (16 are what a ps_hit holds).
 * Not built: -q read trimming and -N (the oracle has neither); the shim refuses them.  ps_map_to_bam, ps_map_profiled and
 * ps_map_route keep the defaults; the route takes the options through ps_map_route_opts (ps_route_opts2.search). */
typedef struct {
    uint32_t struct_size;          /* sizeof(ps_search_opts): a caller built against a shorter struct still works, the fields it lacks keep their defaults */
    int32_t max_gap_opens;         /* aln -o  [1]  */
    int32_t max_gap_extensions;    /* aln -e  [-1]: < 1 = k-difference mode (at most 6 extensions, each counts as a difference);
                                      >= 1 = that many, and they do not count as differences */
    int32_t indel_end_skip;        /* aln -i  [5]  */
    int32_t max_del_occ;           /* aln -d  [10] */
    int32_t seed_len;              /* aln -l  [32]; a value >= the read length means no seed */
    int32_t max_seed_diff;         /* aln -k  [2]  */
    int32_t max_entries;           /* aln -m  [2000000] */
    int32_t s_mm, s_gapo, s_gape;  /* aln -M -O -E [3 11 4]; stock mode only: the profile's costs replace them */
    int32_t max_top2;              /* aln -R  [30] */
    int32_t max_alt_hits;          /* samse -n [3] */
} ps_search_opts;
void ps_search_opts_default(ps_search_opts *);
/* host only (needs no device): 0 if every field lies in its range, else 1 and ps_last_error() names the field and its limit.
 * profile_mode != 0: the ranges under an error profile (max_seed_diff).  NULL: the defaults, 0 */
int  ps_search_opts_check(const ps_search_opts *, int profile_mode);
/* ps_map with search options; NULL: ps_map.  The options reach every device worker of the streaming pass */
int  ps_map_opts(int threads, const char *mm, const char *error_profile, const char *indel_profile,
                 const char *ref_fa, const char *fastq, const char *out_sam, const ps_search_opts *opts);

/* ---- staged interface (same code path as ps_map; used by the argv shim, tests and bench.py) ---- */
typedef struct ps_ctx ps_ctx;
typedef struct ps_batch ps_batch;

ps_ctx *ps_ctx_open(const char *ref_fa, int device);                 /* load <ref_fa>.bwt ... into HBM  */
ps_ctx *ps_ctx_clone(ps_ctx *src, int device);                  /* a context on `device` with a device-to-device copy of src's index (what ps_map gives every device after the first) */
ps_ctx *ps_ctx_build(const char *ref_fa, int device, int save_files);/* build the index (GPU), keep it resident */
void    ps_ctx_close(ps_ctx *);
/* the ranges of ps_map's mm apply; a model outside them fails at ps_batch_from_fastq / ps_batch_from_codes */
int     ps_ctx_set_stock(ps_ctx *, const char *n_arg);               /* bwa aln -n */
int     ps_ctx_set_profile(ps_ctx *, const char *error_profile, const char *indel_profile, const char *x_arg);
int     ps_ctx_set_profile_matrix(ps_ctx *, const double P[16], double ins_rate, double del_rate, int x);
/* the search options are a part of the context of their own: ps_ctx_set_stock / ps_ctx_set_profile* replace the cost part and keep
 * them, in either order of calls.  NULL: back to the defaults.  Checked here under the cost part in force, and again by a later
 * ps_ctx_set_profile* (max_seed_diff 512..4095 is stock only); batches made afterwards search with them */
int     ps_ctx_set_search(ps_ctx *, const ps_search_opts *);
int     ps_ctx_set_tiers(ps_ctx *, const uint32_t pool_cap[3], const int32_t aln_cap[3], int bt_blocks);
/* measurement runs: the search kernel of the following launches counts its search steps, pushes, pops ... and walks the plain Occ
 * blocks (no jump table): the counts are those of the reference algorithm (ps_batch_kstats, which = 1).  The default kernel
 * keeps two counters only -- occ_pairs / occ_same_blk of the steps IT takes through the Occ array (the rest go through the
 * jump table) -- and leaves the others zero */
int     ps_ctx_set_stats(ps_ctx *, int on);
/* lanes of work (stream + workspace) the batches created afterwards take in turn: 1 (default) or 2 -- two batches on two lanes may
 * be driven from two threads at once, one's selection / SA walk / DP stages then run under the other's search kernel */
int     ps_ctx_set_lanes(ps_ctx *, int n);
/* collapsed search: the identical reads of a batch (same bases, same N positions, same length; a read and its reverse complement
 * are different reads) are searched once and the result is copied to the others -- what a pipeline runs a collapsing tool in front
 * of the mapper for.  Every output (hit lists, hits, SAM) stays byte for byte what it is without: names, qualities and the
 * tie-break stream come after the search, in input order.  mode -1 (default): as the environment says when the batch is searched
 * (PS_COLLAPSE=1: on; unset: off), 0 off, 1 on.  Off, no kernel and no buffer of the feature is used.  Declined (searched as if
 * off) under PS_READ_ITERS, whose per-read profile is in launch order.  With ps_ctx_set_stats on, the counters count what ran:
 * the searches of the representatives, not of every read. */
int     ps_ctx_set_collapse(ps_ctx *, int mode);

typedef struct {                       /* index geometry + build facts */
    uint64_t seq_len, l_pac, primary, L2[5], n_blocks, n_sa, device_bytes;
    int32_t n_contigs, n_holes, sa_rounds, sa_intv;
    double build_ms;
    int32_t  jump_levels, pad_;        /* levels of the jump table derived from the index on the device (0: none) */
} ps_index_info;
int     ps_ctx_info(ps_ctx *, ps_index_info *out);
/* index blobs (0 Occ blocks, 1 sampled SA, 2 pac) for the one-off RCCL broadcast over xGMI */
int     ps_ctx_blob(ps_ctx *, int which, void **dev_ptr, uint64_t *bytes);
int64_t ps_ctx_meta(ps_ctx *, char *buf, int64_t cap);               /* serialised contig/hole table + scalars */
ps_ctx *ps_ctx_from_blobs(const char *meta, int64_t meta_len, int device, void *const dev_ptrs[3]); /* borrowed device memory */
int     ps_ctx_fetch(ps_ctx *, int which, void *host_dst, uint64_t bytes); /* D2H copy of a blob (tests) */
int     ps_ctx_export_blob(ps_ctx *, int which, void *dev_dst, uint64_t bytes); /* D2D copy into caller memory (broadcast source) */
int     ps_ctx_index_check(ps_ctx *, uint64_t out[4]);   /* every row of the index checked against the packed text along the LF cycle: rows visited (== seq_len + 1), BWT symbol mismatches, SA sample mismatches, longest arc */
int     ps_ctx_sa_lookup(ps_ctx *, const uint64_t *rows, int64_t n, uint64_t *out); /* SA[row], rows in [1, seq_len]: index checks from the text */
int     ps_ctx_order_sort(ps_ctx *, const uint8_t *keys, int64_t n, int32_t *order); /* the hand-out order of a search launch from its 8-bit keys: order[queue position] = read, a stable ascending sort (tests) */

ps_batch *ps_batch_from_fastq(ps_ctx *, const char *fastq);
ps_batch *ps_batch_from_codes(ps_ctx *, int64_t n, int len, const uint8_t *codes); /* [n][len], 0..3 ACGT, 4 N */
void      ps_batch_free(ps_batch *);
int64_t   ps_batch_n(ps_batch *);
int       ps_batch_search(ps_batch *);                               /* width + backtracking kernels */
int       ps_batch_select_hard(ps_batch *, uint64_t draws_before, uint64_t *draws_after);
int       ps_batch_select_easy(ps_batch *, int threads);
int       ps_batch_locate(ps_batch *);                               /* SA walk + MAPQ + banded DP kernels */
int       ps_batch_run(ps_batch *, int threads);                     /* the four stages above, single process */
int       ps_batch_write_sam(ps_batch *, const char *path, int with_header, int threads);

typedef struct { uint64_t k, l; uint16_t score, units; uint8_t n_mm, n_gapo, n_gape, n_ins, n_del, pad[7]; } ps_aln;   /* 32 B */
typedef struct {
    int64_t pos; uint64_t sa; int32_t type, strand, mapq, n_mm, n_gapo, n_gape, ref_shift, score, c1, c2,
            n_cigar, n_multi; uint32_t cigar[16];
} ps_hit;
typedef struct {
    double ms_width, ms_backtrack, ms_compact, ms_select, ms_sa2pos, ms_refine, ms_host_post, ms_total;
    int32_t n_width_launches, n_backtrack_launches;
    int64_t n_overflow_tier1, n_overflow_tier2;
    double ms_classify, ms_rows, ms_sel_hard, ms_sel_easy;   /* host sub-stages */
    double bt_begin_ms, bt_end_ms;   /* the search launches of this batch on the context's clock: two batches on two lanes overlap */
} ps_timing;
typedef struct { uint64_t occ_pairs, occ_same_blk, nodes, pushes, pops, lf_steps, iters, exact_steps; } ps_kstats;

int     ps_batch_n_aln(ps_batch *, int32_t *out, int64_t cap);       /* per read, input order */
int64_t ps_batch_alns(ps_batch *, int64_t read, ps_aln *out, int64_t cap);
int     ps_batch_hits(ps_batch *, ps_hit *out, int64_t cap);
int     ps_batch_timing(ps_batch *, ps_timing *out);
int64_t ps_ctx_read_iters(ps_ctx *, uint32_t *out, int64_t cap);   /* profiling aid (env PS_READ_ITERS=1): per read of the last search launch 20 words -- iterations | stack slots used | lower bounds as fetched (read, seed << 8) and the effort estimate's two scans (<< 16, << 24) | best score, final budget << 8, hits << 16 | 16 words of D bounds -- in the order the launch held the reads (leading-base order of the bin, not input order); returns the word count */
int64_t ps_ctx_launch_order(ps_ctx *, uint8_t *est, uint8_t *key, float *pred, int32_t *order, int32_t *ids, int64_t cap);   /* profiling aid (env PS_READ_ITERS=1): what the last search launch was prepared with, per read by the index ps_ctx_read_iters rows have -- the estimated best score in budget units, the 8-bit class the hand-out order sorts by, the expected number of search nodes it was made from (0 under PS_ORDER=2), queue position -> read, and read -> input read; null pointers are skipped; returns the number of reads, 0 where the launch made no order */
int     ps_batch_kstats(ps_batch *, int which /*0 width 1 backtrack 2 sa2pos*/, ps_kstats *out);
/* what the collapsed search (ps_ctx_set_collapse) found and saved, after ps_batch_search.  The groups are EXACT: two reads share a
 * group only after all their packed words and their length have compared equal, never on a hash alone.  They may be INCOMPLETE in
 * one rare case: identical reads are found as neighbours in an order sorted by a 64-bit key, and where reads of equal key and
 * different sequence interleave there, identical reads end up in two groups -- that costs a search, never a wrong result.
 * Searched with collapse off: n_searched == n_reads and the rest 0. */
typedef struct {
    int64_t n_reads, n_searched;            /* first tier, all bins: reads, and reads that were actually searched */
    int64_t n_groups, n_multi, largest;     /* groups, groups with more than one read, reads in the largest group */
    int64_t n_overflow_reads, n_overflow_searched;   /* larger tiers, summed: reads that needed one, reads searched there */
    int32_t n_bins, n_bins_collapsed;       /* bins of the batch, bins where a duplicate was found */
    double  ms_collapse;                    /* key, sort, heads, gather and expand kernels, all bins */
} ps_collapse_info;
int     ps_batch_collapse_info(ps_batch *, ps_collapse_info *out);
/* the groups, in input order: out[g] = input index of the representative of g's group (a representative names itself), for the
 * first min(cap, n) reads; an error if the batch was not searched or was searched with collapse off */
int     ps_batch_duplicate_of(ps_batch *, int64_t *out, int64_t cap);
/* host-only check of the read parser: whole file on `threads` threads (chunk_bytes 0) or streamed in windows of chunk_bytes as
 * ps_map does; out = {reads, bases, order-sensitive hash of names / sequences / qualities, pieces}.  reads_path: plain, gzip or
 * BGZF as for ps_map, with the same two deviations (a truncated member and trailing bytes are errors); for a compressed input
 * the piece count is the one of an input whose size is unknown */
/* the library keeps up to 3 GB of page-locked host buffers between calls (locking and unlocking them costs ~0.1 s per piece of a
 * ps_map call); this gives them back */
void    ps_release_host_cache(void);
int     ps_parse_check(const char *reads_path, int threads, uint64_t chunk_bytes, uint64_t out[4]);

/* ---- after the map step --------------------------------------------------------------
 * One call for what PARAsuiteMapping.java:102-133 (`samtools view -bS -t ref x.sam -o x.bam`, `samtools view -q <mapq> -b`)
 * and Mapping.java:85-108 (`samtools sort`, `samtools index`) spawn four processes for: SAM text -> BAM, records with
 * MAPQ < min_mapq dropped, optionally sorted by coordinate (unplaced reads last, input order kept among equals) with
 * <bam>.bai next to it.  Host code (zlib); needs no GPU. */
typedef struct { uint64_t n_in, n_out, bam_bytes; } ps_bam_stats;
int     ps_sam_to_bam(const char *sam, const char *bam, int min_mapq, int sort_by_coordinate, int write_index, int threads,
                      ps_bam_stats *stats /* may be NULL */);
/* ps_map and the steps above in ONE call, without the SAM text in between (PARAsuiteMapping.java:63-152 end to end: `bwa parasuite|aln`,
 * `bwa samse`, `samtools view -bS`, `view -q`, and Mapping.java:85-108's sort + index): alignment records -> BAM records -> BGZF, piece by
 * piece while later pieces of the input are searched.  out_bam holds the records with MAPQ >= min_mapq in input order, or sorted by
 * coordinate (+ <out_bam>.bai with write_index).  Record for record what ps_sam_to_bam(ps_map(...)) writes. */
int     ps_map_to_bam(int threads, const char *mm, const char *error_profile, const char *indel_profile, const char *ref_fa, const char *fastq,
                      const char *out_bam, int min_mapq, int sort_by_coordinate, int write_index, ps_bam_stats *stats /* may be NULL */);
/* the same steps one by one on BAM input, as the unmodified Java issues them (an argv-compatible `samtools` for exactly
 * these four command shapes is built as para-suite_amd/bin/samtools):
 *   samtools view -q <mapq> -b in.bam -o out.bam   (PARAsuiteMapping.java:121-133)
 *   samtools sort [-n] in.bam -o out.bam            (Mapping.java:86-93, 118-126; -n: names ordered as samtools does)
 *   samtools index in.bam                           (Mapping.java:100-105)  -> in.bam.bai, the BAM is not rewritten */
int     ps_bam_view(const char *in_bam, const char *out_bam, int min_mapq, int threads, ps_bam_stats *stats);
int     ps_bam_sort(const char *in_bam, const char *out_bam, int by_name, int threads, ps_bam_stats *stats);
int     ps_bam_index(const char *bam, int threads);

/* ---- between the two mapping passes -------------------------------------------------------
 * What `new ErrorProfiling(mapping, reference, maxReadLength).inferErrorProfile(false, false)` writes for the second pass
 * (src/src/utils/errorprofile/ErrorProfiling.java:100-631, called at src/src/main/Main.java:327-334): counted on the GPU over
 * the records of the first pass's SAM or BAM file (unmapped, duplicate and position-less records skipped, :155-166; counts
 * in read orientation, :301-306,376-377), against the reference of an existing index (<ref_fa>.pac/.ann):
 *   <out_prefix>.errorprofile  4 lines x 4 values, row = reference base, each Double.toString + TAB (NaN if never seen), :504-531
 *   <out_prefix>.indelprofile  "<ins>\t<del>" without newline, :545-591
 * out_prefix NULL or "": the mapping file's name, as in the Java.  A read longer than max_read_len is an error (the
 * Java's arrays would overflow).  max_read_len 1..2275 (the counting kernel's LDS, 160 KiB at 18 words per position); the
 * same range holds for ps_map_profiled and for max_read_len of ps_route_opts.  Outside it the call fails and writes nothing. */
int     ps_error_profile(const char *mapping_sam_or_bam, const char *ref_fa, int max_read_len, const char *out_prefix);
/* Everything `new ErrorProfiling(mapping, reference, maxReadLength).inferErrorProfile(infer_qualities, false)` writes -- the
 * toolkit's `error MAPPING REF MAXLEN [-q true]` mode (Main.java:560-597), whose .qualities and .indels feed the PAR-CLIP
 * simulator's quality_file / indel_file.  Same records, rules and reference as ps_error_profile, and:
 *   <out_prefix>.errorprofile, .indelprofile  byte-identical to ps_error_profile with the same arguments
 *   <out_prefix>.errorprofile.vcf   4 blocks (reference base A C G T) of 4 lines "<ref>\t<read>\t<count as Double.toString>",
 *                                   a blank line after each block, :504-531
 *   <out_prefix>.qualityPerMismatch 4 lines x 4 values "mean QUAL\t" (NaN: no pair), pairs of records whose CIGAR has no I
 *                                   and no D, :379-390,438-447
 *   <out_prefix>.indels             max_read_len lines "<ins rate>\t<del rate>" per read position (0.0 where no base), :553-579
 *   <out_prefix>.qualities          max_read_len lines "<mean>\t<sd>" of QUAL per read position (NaN\tNaN where none), the
 *                                   standard deviation summed in file order, :402-406,421-436; created empty when
 *                                   infer_qualities == 0
 * QUAL is Phred (SAM QUAL - 33, BAM bytes), indexed in SAM order and never reversed (:301 takes it before the reverse
 * complement): column i of a reverse-strand record pairs its complemented bases with QUAL[i].  Where the Java throws, this
 * does not, and counts the case in stats:
 *   - deletion and N records with -q: the Java reads QUAL[width - 1] past the read (ArrayIndexOutOfBounds, uncaught); here
 *     positions i < read length are booked;
 *   - reverse-strand N records: their .qualityPerMismatch index can pass the read's end; those pairs are left out and
 *     counted in n_qual_beyond_read;
 *   - QUAL '*' (BAM 0xFF): the Java throws at the first quality; here the record adds nothing to the two quality files,
 *     everything else as before, and is counted in n_without_qual (counted records that are not skipped);
 *   - the Java sums .qualityPerMismatch in a 32-bit int (wraps near 10 M reads); here the sums are exact 64-bit.
 * max_read_len 1..2028 with infer_qualities, 1..2254 without (the counting kernel's LDS, 160 KiB); a read longer than max_read_len is an error, as in
 * ps_error_profile, and no file is written then. */
typedef struct { uint64_t n_records, n_counted, n_unmapped, n_duplicate, n_start_zero, n_indel_reads, n_skipped,
                 n_without_qual, n_qual_beyond_read; } ps_profile_stats;
int     ps_error_profile_full(const char *mapping_sam_or_bam, const char *ref_fa, int max_read_len, const char *out_prefix,
                              int infer_qualities, ps_profile_stats *stats /* may be NULL */);
/* RBP-bound clusters with T->C statistics -- the toolkit's `clust MAPPING REF OUT SNP_VCF MIN_COVERAGE` mode
 * (Main.java:601-639, PileupClusters.calculateReadPileups): the six files of the Java, byte for byte as the plain restatement
 * in tests/java_pileupclusters.py writes them (no JVM is at hand, so this is not pinned to the jar itself):
 *   <out_file>                      cluster table (header with the Java's "Seqenece"), one line per written cluster
 *   <out_file>.ccr.fasta / .ccr.tsv crosslink-centred regions: [best site - 20, best site + 20] of every written cluster
 *                                   with a best site
 *   <out_file>.report               five counter lines ("Loci found that are SNPs" is always 0)
 *   <site_prefix>.sitefrequency.tsv mean k-th largest T->C fraction over crosslinked clusters (the first one's k >= 1 counted
 *                                   twice, as in the Java)
 *   <site_prefix>.sitepositions.tsv per read index 0..50 the share of crosslinked clusters with a T->C there (NaN for none)
 * The input must be coordinate-sorted by its header (@HD SO:coordinate); records with flag 4 are skipped, records whose
 * CIGAR holds (I or D) and N are skipped and counted, and the last cluster is never written (all as in the Java).  Only the
 * header is checked: records that are locally out of order under it are clustered in file order, as the Java would.
 * site_prefix NULL or "": the mapping file's name.  snp_vcf NULL or "": no known SNPs (an extension); the VCF is read whole
 * (plain, gzip or BGZF), so no .tbi is needed.  ref_fa needs its index (.ann/.pac, ps_index); sequence text comes from the
 * FASTA itself, which may be plain, gzip or BGZF like ps_index's (the same string serves both; the index is named after it as
 * given); deviations as for ps_map's reads: a truncated member or bytes behind the last one fail the call.  Where the Java throws or is undefined, this does not, and counts the case in stats instead:
 *   - T->C at read index >= 51 (the Java's boolean[51] throws): counted everywhere but the read-index flags (n_t2c_beyond_51);
 *   - CCR window starting before base 1 (htsjdk reads bytes before the contig): empty CCR sequence (n_ccr_clipped);
 *   - a HashMap bucket of more than 8 sites at the end of a cluster (the Java resizes or makes a tree, and its iteration
 *     order leaves the model): n_order_unmodelled;
 *   - a VCF record whose first ALT allele is '.', '*', symbolic or a breakend never matches.
 * A CCR window past the contig's end gives an empty sequence as in the Java (n_ccr_past_end).  Input that is not
 * coordinate-sorted (the Java writes six empty files and exits 0), a record on a contig the index lacks, a record or a
 * cluster-sequence fetch past its contig's end, and a mapped record with SEQ '*' are errors: nothing is written then.
 * n_clusters_written counts the lines of <out_file>, the MIN_COVERAGE <= 0 line of the empty first pseudo-cluster included. */
typedef struct { uint64_t n_records, n_unmapped, n_skipped_indel, n_kept, n_clusters, n_clusters_written, n_crosslinked, n_ccr,
                 n_double_stranded, n_snp_hits, n_snv_sites, n_t2c_beyond_51, n_ccr_clipped, n_ccr_past_end,
                 n_order_unmodelled; } ps_cluster_stats;
int     ps_pileup_clusters(const char *mapping_sam_or_bam, const char *ref_fa, const char *out_file, const char *snp_vcf,
                           int min_read_coverage, const char *site_prefix, ps_cluster_stats *stats /* may be NULL */);
/* ---- the transcript route of `map -t TRANSCRIPTS.fa` (Main.java:363-416) ----------------------------------------------
 * Step 2, `new ExtractWeakMappingReads().extractReads(mapping, mappingNew, fastq, 10)` (ExtractWeakMappingReads.java:40-94):
 * the records of a SAM or BAM file in file order; one with MAPQ < mapq_threshold becomes four FASTQ lines "@QNAME", SEQ, "+",
 * QUAL ('\n' line ends; with flag 16 SEQ is reverse-complemented as SequenceUtil.reverseComplement does -- A C G T swapped,
 * every other base code kept -- and QUAL reversed, i.e. the read as it was sequenced), every other record goes to out_bam
 * unchanged under the input's header and reference table (what ps_bam_view keeps at that threshold).  Host code (zlib);
 * needs no GPU.  out_bam and out_fastq may not be the input file: the caller renames, as Main.java:376-377 does.
 * Deviations: a weak record with SEQ '*' or without QUAL is an error naming the record (the Java writes a FASTQ no parser
 * takes), and nothing is left behind then; SEQ comes out in upper case (BAM's 4-bit codes). */
typedef struct { uint64_t n_records, n_weak, n_kept, bam_bytes; } ps_extract_stats;
int     ps_extract_weak_reads(const char *mapping_sam_or_bam, const char *out_bam, const char *out_fastq,
                              int mapq_threshold, int threads, ps_extract_stats *stats /* may be NULL */);
/* The toolkit's `extractAligned -a MAPPING -o OUT` mode (Main.java:852-880), `ExtractNotMappedReads.extractReads`
 * (src/src/utils/postprocessing/ExtractNotMappedReads.java:33-88): one line "@" + QNAME + "\n" per record of the SAM or BAM file, in
 * file order, whatever the flags.  Host code; needs no GPU.  Written under <out_file>.names-tmp and renamed; an error leaves
 * nothing behind, and an output that is the input is refused. */
typedef struct { uint64_t n_records, out_bytes; } ps_names_stats;
int     ps_extract_read_names(const char *mapping_sam_or_bam, const char *out_file, ps_names_stats *stats /* may be NULL */);
/* Step 5 and the toolkit's `comb -g GENOMIC -t TRANSCRIPT -o OUT` mode (Main.java:438-488),
 * `new CombineGenomeTranscript().combine(genome, transcript, out)` (CombineGenomeTranscript.java:36-666): out_bam holds all
 * genomic records in file order, then the transcript hits lifted to genome coordinates in transcript-file order, under the
 * genomic file's header and reference table.  Both inputs are SAM or BAM.  The lift runs on the GPU; the rules are those of
 * the Java as it is written, restated in plain Python in tests/java_combine.py (no JVM is at hand to pin it to the jar):
 *   - the transcript file must be SO:queryname by its header, else an error and nothing is written (the Java logs, exits 0);
 *   - records with RNAME '*' are passed over (n_unplaced); they neither break nor start a name group;
 *   - the transcript's name is split on '|': field 2 chromosome without "chr", 3 exon starts and 4 exon ends (';'-separated,
 *     EACH SORTED AS STRINGS -- Arrays.sort(String[]), so "100000" sorts before "99990"), 5 strand; parsed once per transcript
 *     that a record names.  Fewer than six fields, an exon that is not an int, or unequal counts: an error naming the transcript;
 *   - strand "1" (:211-390) walks the exons upwards, "-1" (:391-518) downwards: start = exonStart + (alnStart - passedBefore) - 1,
 *     on -1 the end is exonEnd - (alnStart - passedBefore) + 1.  A read inside one exon keeps its own CIGAR (on -1 its start is
 *     end - READ LENGTH + 1, not the reference span); a read across junctions gets xM yN ... zM.  An intron of length <= 0 or a
 *     run past the last exon ends the walk with what was built.  A read across a junction with I or D in its CIGAR is counted in
 *     n_missed_indel_splice: on "1" it is still emitted with the CIGAR built so far (possibly none: '*'), on "-1" its start is
 *     still -1 and it is dropped.  Any other strand string locates nothing.  Records without a start: n_unlocated;
 *   - this library's rule for getAlignmentEnd: alignment start + reference length of the CIGAR - 1, and 0 for a record with
 *     flag 4 (bwa's bridging records keep RNAME, POS and CIGAR; htsjdk 1.128 answers 0 for an unmapped record, as far as the
 *     maintainers remember it).  Worked cases, exons 1000-1099 and 2000-2099, strand "1": a flag-4 record at POS 91 with 20M
 *     lies in exon 0, 0 <= 100 ends the walk there and it is located at 1090 with its own 20M, not 10M1900N10M; the same
 *     record at POS 150 finds no start in exon 0 (150 > 100), 0 <= 100 ends the walk and it stays unlocated;
 *   - a group is a maximal run of equal QNAME among the records with a reference.  Its located records, in file order, form a
 *     list; unequal lifted starts: the group emits nothing (n_groups_ambiguous); else ONE record is emitted, the list entry
 *     whose index was last stored by a record without flag 0x100 (entry 0 if there was none), with its own start and CIGAR;
 *   - the contig is "chr" + field 2; absent from the genomic header: nothing emitted (n_no_contig).  "MT" is looked up as
 *     "chrMT" FIRST (the Java's order), then placed on "chrM"; without chrM the record is written with reference id -1 and its
 *     lifted position (n_mt_unplaced);
 *   - the emitted record: new reference id, POS, CIGAR, bin, MAPQ 10; for strand "-1" flag 16 toggled and SEQ
 *     reverse-complemented, QUAL NOT reversed (as in the Java); name, other flags, mate fields and tags unchanged.
 * n_spliced counts located records (emitted or not) whose lifted CIGAR holds an N (:539-541); n_groups the name groups.
 * Deviations: (1) htsjdk's writer would always sort here (the header says coordinate, presorted is false); the unsorted form
 * (sort_by_coordinate 0) is this library's own; it carries the genomic header as it is, @HD SO: NOT rewritten, so a genomic
 * file that says SO:coordinate yields an unsorted output that still says so -- sort it (or ask for the sorted form) before a
 * tool that trusts @HD reads it.  With sort_by_coordinate the sequence above is sorted stably, byte for byte
 * what ps_bam_sort makes of the unsorted output; write_index adds <out_bam>.bai.  (2) A lifted start below base 1 other
 * than -1 (a flag-4 record beyond the last exon of a "-1" transcript gets -READ LENGTH) is treated like -1: the Java would
 * hand htsjdk a record before its contig's first base.  (3) Errors where the Java throws (above) write nothing.
 * Without a HIP device the call fails. */
typedef struct { uint64_t n_genome, n_transcript, n_unplaced, n_unlocated, n_missed_indel_splice, n_groups,
                 n_groups_ambiguous, n_no_contig, n_mt_unplaced, n_lifted, n_spliced, n_strand_flipped, bam_bytes; } ps_combine_stats;
int     ps_combine_genome_transcript(const char *genome_bam, const char *transcript_bam, const char *out_bam,
                                     int sort_by_coordinate, int write_index, int threads, ps_combine_stats *stats /* may be NULL */);
/* The first pass and its error profile in one call -- "fed directly from alignment results" (SURVEY.md §8f rank 4): ps_map, and
 * while the SAM is written the same records, straight from memory, go through the counting kernel: the alignments with
 * MAPQ >= min_mapq, i.e. what the pass's filtered BAM holds (samtools view -q, PARAsuiteMapping.java:124-133 /
 * BWAMapping.java) and ErrorProfiling would read back (Main.java:327-334).  Writes <profile_prefix>.errorprofile and
 * .indelprofile, the same bytes as ps_error_profile on that filtered file.  No BAM round trip between the passes. */
int     ps_map_profiled(int threads, const char *mm, const char *error_profile, const char *indel_profile,
                        const char *ref_fa, const char *reads_fq, const char *out_sam,
                        int min_mapq, int max_read_len, const char *profile_prefix);

/* ---- the whole `map` mode in one call (Main.java:249-420, BWA and PARA-suite mappers) -----------------------------------------
 * `-q READS -r REF [-t TRANSCRIPTS] -o PREFIX [--refine]`: the stock pass, the error profile of its records, the profile pass,
 * the weak-read extraction, the transcript pass, the name sort, the lift and the coordinate sorts with their indexes, leaving
 * the files Main.java names (<P> = out_prefix; "sorted" = by coordinate with a .bai next to it):
 *   no refine, no transcripts   <P>.BWA-genomic.bam sorted (MAPQ >= mapq_genomic)
 *   no refine, transcripts      <P>.BWA-genomic.bam sorted (the records the extraction keeps), <P>.BWA-transcript.bam sorted by name
 *                               (MAPQ >= mapq_transcript), <P>.combined.bam sorted
 *   refine                      <P>.BWA-genomic.bam sorted, <P>.BWA-genomic.bam.errorprofile / .indelprofile, <P>.PARAsuite-genomic.bam
 *                               sorted; with transcripts also <P>.PARAsuite-transcript.bam and <P>.combined.bam
 *   refine with error_profile   no first pass and no profile files of its own; the rest as the refine rows
 * Every file holds what the calls above write under that name when issued one by one (ps_map_to_bam; ps_error_profile on the
 * filtered first-pass BAM; ps_map_to_bam with the two profile files; ps_extract_weak_reads and the rename; ps_bam_sort and
 * ps_bam_index; ps_map_to_bam on the weak FASTQ against the transcripts; ps_bam_sort -n; ps_combine_genome_transcript sorted and
 * indexed): BAMs record for record, header included, profile files byte for byte.  Inside the call the reads file is parsed once
 * (the parsed pieces stay in host memory for the profile pass, up to PS_ROUTE_KEEP_MB megabytes -- default 8192; a
 * larger input is parsed again, with the same output), each index is loaded once and stays in HBM with its lanes of work until the
 * call returns (the transcript pass takes over the genome passes' lanes), the weak reads go to the transcript pass from memory
 * (names as a second parse leaves them: one more trailing /1 or /2 removed), and no BAM is written to be read back.  Each pass is
 * a samse run of its own (its tie-break stream starts at 0).  ps_index runs for a reference whose .bwt is missing.  Nothing stays
 * resident when the call returns, unless a resident scope is open (below).
 * Errors before anything is touched: error_profile without refine (nothing to map), a missing reads_fq / ref_fa / out_prefix, an
 * output name that is one of the inputs, no HIP device.  FASTA reads with a transcript route fail as ps_extract_weak_reads does on
 * records without QUAL.  On any error ps_last_error() names the step ("first pass", "profile", "refine pass", "transcript pass",
 * "combine") and every file the call created is removed -- outputs are written under <name>.route-tmp and renamed when their
 * step is done -- except index files that ps_index wrote.  "Created" goes by name: a file of an output's name left by an earlier
 * run is overwritten when its step is done and removed with the rest when a later step fails.  An indel_profile without an
 * error_profile is refused too, and an output's temporary name counts as the output where the inputs are compared.
 * stats: first / refine / transcript are the stats of the BAM each pass left (zeros for a pass that did not run; bam_bytes of the
 * file as written here); extract.bam_bytes is 0 (no intermediate BAM exists); n_index_loads_*: how often an index was read from its
 * files (1 per reference used); n_fastq_parses: 1, or 2 when the input exceeded PS_ROUTE_KEEP_MB.  PS_VERBOSE=1 prints the stage times. */
typedef struct {
    const char *reads_fq, *ref_fa, *out_prefix;      /* -q -r -o : required */
    const char *transcripts_fa;                      /* -t ; NULL or "": no transcript route */
    const char *bwa_mm, *parasuite_mm;               /* --bwa-mm ("2"), --parasuite-mm ("-1"); NULL: those defaults */
    const char *error_profile, *indel_profile;       /* --parasuite-ep / --parasuite-indel: given => no first pass (Main.java:193-203) */
    int32_t threads, refine, max_read_len, mapq_genomic, mapq_transcript;   /* -p, --refine, -l (101), --gm (10), --tm (1); <= 0 where a default exists: the default */
} ps_route_opts;
typedef struct {
    uint64_t n_reads;
    ps_bam_stats first, refine, transcript;          /* the BAM each pass left; zeros for a pass that did not run */
    ps_extract_stats extract; ps_combine_stats combine;
    double s_total, s_parse, s_index_genome, s_index_transcripts, s_first, s_profile, s_refine, s_transcript, s_combine;
    uint32_t n_index_loads_genome, n_index_loads_transcripts, n_fastq_parses, pad_;
} ps_route_stats;
int     ps_map_route(const ps_route_opts *opts, ps_route_stats *stats /* may be NULL */);
/* The route with an options struct that can grow: everything ps_route_opts holds, and Main.java's --ref-refine and --unaligned and the
 * search options.  struct_size as in ps_search_opts: a multiple of 4; a shorter struct keeps the defaults of the fields it lacks; a
 * longer one is refused, and so is one that ends inside a pointer.  ps_map_route(o) is this call with ref_refine NULL,
 * keep_unaligned 0 and search NULL: the same code, the same bytes.  <P> = out_prefix, Q = mapq_genomic, U = <P>.unaligned.fastq.
 * ref_refine (--ref-refine, Main.java:219-225, :318): means something with refine only and is ignored without it (the Java assigns
 *   it inside `if (isRefine)`).  The first pass maps against ref_fa; from then on everything uses ref_refine: the error profile of
 *   the first-pass BAM is taken against it (:327-329; contigs matched by name, as ps_error_profile does, whose path on the written
 *   file this is: it maps <ref_refine>.pac beside the index load), and the refine pass maps against it.  ps_index runs for it when its
 *   .bwt is missing.  The transcript pass is unchanged.  NULL or "": ref_fa.  Each index is loaded once: n_index_loads_genome is 2
 *   when the two references differ by realpath and 1 otherwise (1 also with a given error_profile: no pass maps against ref_fa
 *   then, and only ref_refine is loaded).  A first-pass record on a contig ref_refine lacks fails the call at
 *   step "profile", and nothing is left behind.
 * keep_unaligned (--unaligned, :226-229, :354-357, :382-390, :405-407):
 *   refine, no transcripts   the refine pass is written unfiltered (MAPQ 0) and sorted, then the extraction of :382-388 runs on the
 *                            sorted file: U holds the records with MAPQ < Q in the sorted file's order, byte for byte what
 *                            ps_extract_weak_reads writes from that file, and <P>.PARAsuite-genomic.bam the records it keeps, still
 *                            sorted.  Deviation: the Java leaves the .bai it wrote before the rewrite, which no longer fits the
 *                            file; here the .bai is written for the file as it ends up;
 *   no refine, no transcripts  the first pass has already dropped MAPQ < Q (:284-291): U is created empty and the BAM is unchanged,
 *                            as in the Java;
 *   transcripts              as written, the second extraction (:382-388) runs on the already filtered BAM and overwrites U with
 *                            nothing before the transcript pass reads it (:398), which then maps an empty file.  Deviation: the
 *                            second extraction is not made; U of the first extraction (:299-302 or :371-374) is kept instead of
 *                            removed (:405-407): what ps_extract_weak_reads writes there, in that file's (the input's) order.
 *                            Every other file is what the call writes without the flag.
 *   U is published like the route's other outputs and counts as an output where inputs and outputs are compared.
 * search: the options of every mapping pass of the call (first, refine, transcript); NULL: the defaults.  Ranges and refusals are
 *   those of ps_map_opts, checked before anything is touched (under the profile's ranges too when a profile pass will run); s_mm,
 *   s_gapo and s_gape act on the stock-cost passes only.  "Issued one by one" above then reads ps_map_opts(.., search) +
 *   ps_sam_to_bam where it says ps_map_to_bam.
 * A resident scope treats this call as it treats ps_map_route. */
typedef struct {
    uint32_t struct_size;                            /* sizeof(ps_route_opts2) */
    int32_t threads, refine, max_read_len, mapq_genomic, mapq_transcript;   /* as in ps_route_opts */
    const char *reads_fq, *ref_fa, *out_prefix;
    const char *transcripts_fa;
    const char *bwa_mm, *parasuite_mm;
    const char *error_profile, *indel_profile;
    /* -- a struct_size up to here: ps_route_opts -- */
    const char *ref_refine;                          /* --ref-refine; NULL or "": ref_fa */
    const ps_search_opts *search;                    /* NULL: the defaults */
    int32_t keep_unaligned, pad_;                    /* --unaligned */
} ps_route_opts2;
int     ps_map_route_opts(const ps_route_opts2 *opts, ps_route_stats *stats /* may be NULL */);

/* ---- the resident scope: indexes and lanes of work stay in HBM between calls ---------------------------------------------------
 * Outside a scope every mapping call loads its index, allocates its search workspace and frees both before it returns.  Between
 * ps_resident_begin and ps_resident_end (one scope per process, opt-in) ps_map, ps_map_opts, ps_map_to_bam, ps_map_profiled and
 * ps_map_route find their index in HBM where an earlier call of the scope loaded it, find the device's lanes of work (streams,
 * search workspace) allocated, and leave both in place; ps_map_route's "nothing stays resident" holds outside a scope only, and
 * its n_index_loads_* count what THIS call read from files (0 for an index it found).  The output of a call is what it is
 * outside a scope, byte for byte: the cost and search options are set per call, each call is a samse run of its own.
 * An entry is kept under: the reference as realpath names it; the devices and workers per device (PARASUITE_GPUS,
 * PARASUITE_GPU_IDS, PS_WORKERS_PER_GPU); and PS_JUMP, PS_JUMP_LEVELS, PS_POOL_CAP, PS_N_BIG, PS_BT_BLOCKS as they were read.  A
 * call under another key makes another entry.  Beside the key an entry remembers device, inode, size and mtime (nanoseconds) of
 * the four index files: a call that finds them changed closes the entry and loads afresh (n_stale_reloads); ps_index drops the
 * entries of the path it is about to write.  At most max_references entries are held, the least recently used one is closed for
 * a new one (n_evictions).  A device has ONE set of lanes whatever the number of entries: a call moves them to the entry it
 * uses.  A call that fails, for whatever reason, drops every entry it used (n_dropped_after_error); the next call loads afresh.
 * Everything that leaves -- evicted, stale, dropped, and all at ps_resident_end -- is closed on the calling thread before the
 * operation returns (device memory freed, streams destroyed, the .pac unmapped): when ps_resident_end returns no thread of the
 * library touches a device.  A process that exits inside a scope makes no device call from an exit handler.
 * Calls inside a scope take their turn: a second thread's mapping call waits for the first's.  The staged ps_ctx_* interface,
 * the analysis modes and the shims are not part of it.
 * ps_resident_opts.struct_size as in ps_search_opts: a multiple of 4; a shorter struct keeps the defaults of the fields it lacks, a
 * longer one is refused.  Status 1 with ps_last_error(): begin inside an open scope, end without one, max_references outside 1..8. */
typedef struct { uint32_t struct_size; uint32_t max_references; /* [2]; 1..8 */ } ps_resident_opts;
typedef struct {
    uint32_t active, n_references;               /* a scope is open; entries held now */
    uint64_t n_calls, n_index_loads, n_index_reuses, n_stale_reloads, n_evictions, n_dropped_after_error;
    uint64_t bytes_index_resident;               /* sum of the blobs of the held entries, all devices */
} ps_resident_stats;
int     ps_resident_begin(const ps_resident_opts *);  /* NULL: defaults.  Needs no device, makes no device call */
int     ps_resident_end(void);
int     ps_resident_info(ps_resident_stats *);        /* any time; outside a scope: active 0, counters of the last scope */

/* ---- after the mapping: the toolkit's `benchmark MAPPING OUT.stats READS.fastq` mode (Main.java:489-521) -------------------------
 * `new ValidateBenchmarkStatisticsPARCLIP().calculateBenchmarkStatistics(mapping, outStatistics, readsFile, onlyBound)`
 * (src/src/utils/benchmarking/ValidateBenchmarkStatisticsPARCLIP.java:43-242): a mapping of simulated PAR-CLIP reads scored
 * against the truth in the read names "..|..|CONTIG|START|END|BOUND-..", counted on the GPU; the rules are those of the Java as
 * it is written, restated in plain Python in tests/java_benchmark.py (no JVM is at hand to pin it to the jar):
 *   - the reads file (:78-103) is plain text, a gzip magic number is an error.  Lines end at "\n", "\r" or "\r\n"
 *     (BufferedReader.readLine); a last line without an end counts, an end at the end of the file adds no line.  EVERY line
 *     that starts with "@SEQ_ID" -- a quality line may -- is split on '|' (trailing empty fields dropped, as String.split
 *     does) and the text of field 5 before its first '-' counts a positive ("1"), a negative ("0") or nothing;
 *   - the mapping is SAM or BAM; every record counts in file order whatever its flags, unmapped and secondary ones too
 *     (:105-163).  QNAME is split the same way; fields 3 and 4 go through Integer.parseInt (one optional sign, ASCII digits,
 *     int32 range).  The first record where that fails ends the count (:177 catches the exception outside the loop): the
 *     records before it are scored, n_processed is its 0-based index, bad_number_record its 1-based one, and the file IS written;
 *   - a record hits when the truth contig equals the reference name ('*' without one), START - 5 <= alignment start and
 *     END + 5 >= alignment end (32-bit wrap-around as in Java).  Alignment start is POS (0 without one); alignment end
 *     follows this library's rule for getAlignmentEnd, stated at ps_combine_genome_transcript above: 0 for a record with flag
 *     4, so a bridging record that keeps RNAME and POS inside the window scores.  A hit counts TP for bound "1", TN for "0";
 *   - before the comparison (:130-143) the truth contig gets "chr" put in front when the reference name of this OR ANY EARLIER
 *     record starts with "chr" and it lacks it, loses a leading "chr" when no record so far had one, and then exactly "chrM"
 *     becomes "chrMT": a chrM contig never scores, a chrMT contig scores from truth M, chrM or chrMT (the Java's quirk);
 *   - out_statistics (:200-225), no newline at its end: "matched correctly:\t<TP+TN>\nreadsProcessed:\t<n>\nall reads:\t<lines/4>
 *     \nprecision:\t<f>\nrecall:\t<f>\naccuracy:\t<f>" with FP = positives - TP, FN = negatives - TN, (float)TP / (TP + FP),
 *     (float)TP / (TP + FN), (float)(TP + TN) / (positives + negatives) in Java int and float arithmetic (NaN for 0/0,
 *     Infinity for x/0), each as Float.toString writes it (the JDK 19+ definition: the shortest decimal that reads back).
 * Deviations, all where the Java dies or misleads: a "@SEQ_ID" line or a QNAME with fewer than six fields, or whose field 5 is
 * made of '-' only (uncaught ArrayIndexOutOfBounds), is an error naming the 1-based line or record -- for a record only when
 * no unparsable number ended the count before it; a line count that is no multiple of 4 (the Java logs and exits 0 without a
 * file) and a count above 2^31 - 1 (the Java's ints wrap) are errors; nothing is written then.  The Java's "TP=..; TN=.." line
 * on stdout is not reproduced: PS_VERBOSE=1 prints it to stderr with the stage times.  --only-bound is parsed by the Java and
 * never used (:120-125), so it is no parameter here.  Records that score nothing are counted by the first reason that applies
 * (n_unplaced .. n_other_bound below); that breakdown is this library's own and does not enter the file.
 * PS_BENCH_PIECE: bytes of the reads file per staged piece (default 64 MiB; the counts do not depend on it).
 * Without a HIP device the call fails. */
typedef struct {
    uint64_t n_lines, n_reads, n_positives, n_negatives;     /* FASTQ pass: lines, lines / 4, "@SEQ_ID" lines with bound "1" / "0" */
    uint64_t n_records, n_processed, n_tp, n_tn;             /* records in the file; the Java's readsProcessed; truePositives; trueNegatives */
    uint64_t n_unplaced, n_other_contig, n_outside, n_other_bound; /* why a processed record scored nothing: reference '*'; names differ; the +-5 window fails; bound neither "0" nor "1" (first reason that applies, in this order) */
    uint64_t bad_number_record;                              /* 1-based index of the record whose start/end did not parse and ended the count; 0: none */
    float precision, recall, accuracy;                       /* as written to the file */
} ps_benchmark_stats;
int     ps_benchmark_reads(const char *mapping_sam_or_bam, const char *out_statistics, const char *reads_fq,
                           ps_benchmark_stats *stats /* may be NULL */);

/* ---- before the mapping: the toolkit's `simulate TRANSCRIPT_FILE OUTPUT_PREFIX ERROR_PROFILE T2C_PROFILE T2C_POSITIONS_PROFILE
 * QUALITY_DIST INDEL_PROFILE RBP_BOUND` mode (Main.java:684-802, which hands the eight arguments to
 * bin/createSimulatedPARCLIPDataset.pl in that order): PAR-CLIP reads drawn from transcripts on the GPU.  Writes the five files
 * the Perl opens (:35-39): <out_prefix>.fastq, .clusters (the truth of the cluster benchmark), _snps.vsf, .log and .err.  The
 * rules are those of the Perl as it is written, restated in plain Python in tests/perl_simulator.py, which the library matches
 * byte for byte; the random stream is the library's own (Math::Random's cannot be reproduced, and the files must not depend
 * on how the work is cut):
 *   the stream   - every draw is a pure function draw32(seed, transcript ordinal, cluster ordinal, read ordinal, slot):
 *                  mix = the finalizer of splitmix64; run = mix(seed + 0x9E3779B97F4A7C15);
 *                  unit = mix(mix(run ^ transcript) ^ (cluster << 32 | read)); draw32 = mix(unit ^ slot) >> 32.  Transcripts count
 *                  from 0 in file order; cluster 0 / read 0 is the transcript's own unit, cluster 1..3 / read 0 a cluster's, read
 *                  i + 1 the read named ":i".  Slots -- transcript: 0 selection, 1 number of clusters; cluster: 0-11 reads, 12
 *                  position, 13 / 14 / 15 number of T->C sites / starts / ends, 16 + 12 i starts, 52 + 12 i ends, 88 bound, 89 + k
 *                  the k-th site, 128 + 4 z + {0 SNP, 1 alternative base, 2 zygosity, 3 report} for transcript position z; read: 0
 *                  start, 1 end, and for iteration `it` of the per-base loop 16 + 64 it + {0 test, 1 base for a non-ACGT
 *                  character, 2 SNP passes, 3 indel test, 4 inserted base, 8-19 quality, 20-31 the SNP's extra quality, 32-43 the
 *                  insertion's quality};
 *                - rand() is draw32 / 2^32 as a double; ceil(rand() * k) is 1 + floor(draw32 * k / 2^32) and floor(rand() * k) is
 *                  floor(draw32 * k / 2^32), both in integers (the former differs from Perl only at a draw of 0);
 *                  random_normal(mean, sd) is mean + sd * z with z = (sum of 12 draws - 6 * 2^32) * 2^-32, the product and the sum
 *                  rounded separately, no fused multiply-add and no libm call anywhere; int() truncates toward zero;
 *   transcripts  - lines end at "\n" only (chomp), so a "\r" of a CRLF file is part of the sequence; text before the first header
 *                  is dropped.  THE LAST TRANSCRIPT OF THE FILE IS NEVER SIMULATED: createReads runs when the next header
 *                  arrives (:203-218).  The header is split on '|' (trailing empty fields dropped): field 2 the chromosome, 3
 *                  and 4 the exon starts and ends, ';'-separated and each list sorted numerically on its own, the last field the
 *                  strand (read as a number; == -1 reverses the position list, :242-262).  Field 0 keeps its '>', so read names
 *                  begin "@SEQ_ID:>GENE|" (:611);
 *   selection    - a transcript is used when rand() < select_read; it gets 1..3 clusters of int(N(16, 10)) reads each.  A cluster
 *                  at a position < 10 is skipped: it still takes its cl_<n> number, does not advance the cluster index of the
 *                  read names and writes no .clusters line (:276-281);
 *   clusters     - 1..4 T->C sites, 1..3 starts int(N(pos, 1)), 1..3 ends int(N(pos + 23, 1)); the .clusters line
 *                  "cl_<n>\tchr<chr>\t<start>\t<end>\t<bound>" is built from min(starts) and max(ends) through the exon map,
 *                  swapped on strand -1 (:295-301, :366).  Bound when rand() < bound_prob: the 'T's in [max(starts), min(ends))
 *                  are candidates, and per k one is picked by the weights of the site-positions file at position - max(starts)
 *                  (doubles added in the Perl's order; no draw when one candidate is left), removed, and given rate
 *                  sitefrequency[k] (:316-362, :652-686);
 *   SNPs         - per cluster that is not skipped, over the WHOLE transcript: a position is a SNP with snp_rate, homozygous (1)
 *                  or heterozygous (0.5) with equal chance, its alternative one of the three other bases (none for a character
 *                  that is no ACGT: the Perl's undef); written to _snps.vsf with snp_report; snp<id> counts across the whole
 *                  run whether reported or not (:369-394);
 *   reads        - one of the starts and one of the ends; left out, its ":i" kept, when end - start > 30 or start >= end
 *                  (:412-418).  The per-base loop (:428-591): a T->C site of a bound cluster gives 'C' when rate > test, else
 *                  the base, and moves on; a non-ACGT character writes an .err entry (three lines, the whole sequence among
 *                  them) and takes the error row of a uniformly drawn base, a match still copying the character and a mismatch
 *                  by k giving ACGT[(0 + k) % 4]; a SNP at the position passes with probability 1 or 0.5 and APPENDS an extra
 *                  quality and the alternative base -- the error step still follows, so such a read is one character longer
 *                  (and where the alternative is none, its quality line is); the error step uses the profile row with its
 *                  diagonal replaced by 1 - the other three and thresholds in the order base, +1, +2, +3, a mismatch moving on;
 *                  a match falls through to the indel step when allow_indels: only the first indel of a read counts, an
 *                  insertion (test <= ins[j]) appends a random base with a quality and repeats position j, a deletion
 *                  (<= del[j]) only counts -- the base was appended already.  "bases simulated" counts only iterations that
 *                  reach the loop's end;
 *   qualities    - int(N(mean_j, sd_j)); above 64 becomes 64, at or below 2 becomes 3, the character is 33 + q (:621-633).
 *                  Numbers in the profile files are read as Perl reads a string in numeric context: the decimal number it
 *                  starts with, so the "\r" of a CRLF file is ignored;
 *   read names   - "@SEQ_ID:<field 0>|<field 1>|<chr>|<a>|<b>|<bound>-<cluster index>:<i>" with a, b = gp[start], gp[end] on strand
 *                  == 1 and gp[end] + 1, gp[start] + 1 otherwise (:603-611);
 *   .log         - the eleven counter lines and the two parameter lines (:221-227); divisions as Perl prints numbers (%.15g);
 *                  "read with most T2C" includes the Perl's count of "+2" mismatches (:538).
 * Deviations.  The Perl binds the error row before it replaces a non-ACGT character (:453, :497), so it reads an empty row there;
 * this library takes the row of the drawn base, as the replacement intends.  Where the Perl dies or reads undefined values the
 * call fails, naming the transcript or the file: a run that emits no read (the Perl divides by zero and leaves an empty FASTQ); a
 * header with fewer than six fields, a non-integer exon bound or unequal numbers of starts and ends; exons shorter in total than
 * the sequence (all checked for every transcript but the last, selected or not); a profile file with fewer lines than the loop
 * can index: 4 error rows, 4 site frequencies, 40 site positions, 31 quality lines, 31 indel lines.  On any error nothing is left
 * behind: the files are written under <name>.sim-tmp and renamed together.  The Perl's progress lines are not reproduced;
 * PS_VERBOSE=1 prints the stage times.  Without a HIP device the call fails. */
typedef struct {
    const char *transcripts_fa, *out_prefix, *error_profile, *t2c_profile, *t2c_positions, *quality_dist, *indel_profile;   /* all required */
    double bound_prob;                               /* RBP_BOUND: the fraction of clusters that are bound */
    uint64_t seed;
    double select_read;                              /* <= 0: 0.216, the Perl's $select_read */
    double snp_rate;                                 /* < 0: 0.01 (:377); 0 switches SNPs off */
    double snp_report;                               /* < 0: 0.8, the Perl's $report_snp */
    int32_t allow_indels, pad_;                      /* < 0: 1, the Perl's $allow_indels; 0: no indel step, the indel file is not read */
} ps_simulate_opts;
typedef struct {
    uint64_t n_reads, n_bases_simulated, sum_read_length, n_clusters, n_t2c, n_errors, most_t2c, most_errors, n_indels, n_snps;   /* the .log, in its order (sum_read_length: the numerator of its third line) */
    uint64_t n_transcripts, n_selected, n_clusters_skipped, n_reads_skipped, n_snps_reported, n_non_acgt;   /* headers in the file; transcripts used; clusters at a position < 10; reads left out; _snps.vsf lines; .err entries */
    uint64_t n_snps_preselected, n_snp_positions;    /* SNPs of the pre-selection; (cluster, position) pairs it drew for */
    double avg_read_length, avg_reads_per_cluster;   /* as written to the .log */
    double s_total, s_read, s_plan, s_snp, s_snp_kernels, s_reads, s_write;   /* seconds: the inputs; plan kernel, scans, download; SNP passes with scan and download, and their two kernels alone; read kernel and download; text and files */
} ps_simulate_stats;
int     ps_simulate_reads(const ps_simulate_opts *opts, ps_simulate_stats *stats /* may be NULL */);

/* ---- after `clust`: the toolkit's `fetch -i SITES -r REF -o OUT` (bed == 0) and `fetchBed` (bed != 0) modes (Main.java:883-945) ----
 * `new FetchSequencesForBindingSites().fetchSequences(ref, sites, out)` and `new FetchSequencesForBEDFile().fetchSequences(..)`
 * (src/src/utils/pileupclusters/FetchSequencesForBindingSites.java, FetchSequencesForBEDFile.java): the reference sequence of
 * every site of a table, gathered on the GPU from the index's packed forward strand.  ref_fa names an existing index as for
 * ps_error_profile; only <ref_fa>.ann and <ref_fa>.pac are read (the same string serves a gzip-named reference: genome.fa.gz
 * finds genome.fa.gz.ann), the FASTA itself is not opened and need not exist, and the .fai the Java insists on is not needed.
 * The index keeps every run of non-ACGT letters with its character, and both Java classes upper-case every base they fetch
 * (:64-68), so the soft-masking the index drops never reaches the output.  The rules are those of the Java as it is written,
 * restated in plain Python in tests/java_fetch.py (from the FASTA text; no JVM is at hand to pin it to the jar):
 *   lines      - end at "\n", "\r" or "\r\n" (BufferedReader.readLine); a last line without an end counts, an end at the end
 *                of the file adds no line.  Line 1 is copied to the output, followed by "\n", in BOTH modes (:26-28): in
 *                fetchBed a first BED record is consumed as the header and never fetched.  Every further line is split on
 *                TAB, trailing empty fields dropped (String.split);
 *   fetch      - (the cluster table of `clust`) field 1 is the contig, taken as it is; fields 2 and 3 are start and end,
 *                read by Integer.parseInt; field 4 equal to "-" means reverse, anything else forward.  The sequence REPLACES
 *                FIELD 11 -- on a `clust` table the SeqLength column, not "Seqenece" -- and the fields are joined with TAB
 *                and ended with "\n" (:70-73); fields that split dropped stay dropped;
 *   fetchBed   - field 0 is the contig, with "chr" put in front unless it starts with it (:40-43); fields 1 and 2 go to
 *                getSubsequenceAt UNCHANGED, so BED's 0-based half-open pair is read as 1-based inclusive: one base longer
 *                and shifted; field 4 -- BED's score column, not its strand column -- equal to "-" means reverse.  The
 *                output is ">" + field 3 + "\n" + sequence + "\n";
 *   sequence   - bases start..end of the contig, 1-based and inclusive; for a reverse site SequenceUtil.reverseComplement:
 *                the order reversed, A C G T (either case) swapped, every other character kept; then every character
 *                through toUpperCase.  A base inside a hole is the hole's character, upper-cased (n -> N; R stays R, on
 *                the reverse strand too);
 *   empty      - (SAMException caught, :59-61) a site is left empty when start > end + 1 (in Java ints: end + 1 wraps), when
 *                the contig is not in the index, or when end > contig length; start == end + 1 is a legal empty sequence.
 *                In fetch an empty sequence still replaces field 11, so a line of twelve fields ends in a TAB.
 *   - site starting before base 1 (htsjdk reads bytes before the contig): empty sequence (n_before_start).
 * Deviations, all where the Java dies or misleads: an empty sites file (the Java writes the text "null"); a data line with
 * fewer than 12 fields in fetch or fewer than 5 in fetchBed, a blank line among them (uncaught ArrayIndexOutOfBounds); a start
 * or end that Integer.parseInt refuses (caught outside the loop, the writer never closed: an 8 KB-granular torso remains);
 * out_file equal to an input; a missing index; no HIP device -- each is an error that names the 1-based line or the file, and
 * nothing is left behind: the output is written under <out_file>.fetch-tmp and renamed.  PS_VERBOSE=1 prints the stage times.
 * PS_FETCH_PIECE: bytes of sequence gathered per piece (default 256 MiB, at most 4 GiB, rounded up to a multiple of 16; the
 * pieces are cut anywhere, inside a site too, and the output does not depend on the cut). */
typedef struct {
    uint64_t n_lines, n_sites, n_reverse, n_bases, n_hole_bases;        /* lines read (header included); data lines; strand "-"; bases written; of them from holes */
    uint64_t n_inverted, n_no_contig, n_past_end, n_before_start;       /* sites left empty, by the first reason that applies, in this order */
    uint64_t n_pieces;
    double s_total, s_read, s_index, s_kernels, s_write;
} ps_fetch_stats;
int     ps_fetch_sequences(const char *ref_fa, const char *sites, const char *out_file, int bed, ps_fetch_stats *stats /* may be NULL */);

/* ---- BGZF compression on the device -------------------------------------------------------------------------------
 * Every BAM the library writes is a sequence of BGZF blocks: gzip members of at most 0xff00 input bytes, each its own DEFLATE
 * stream with its own CRC32.  By default they are compressed with zlib on host threads.  The device switch: -1 (the default)
 * is host zlib; device >= 0 means that every BAM this process writes from now on -- the sam_to_bam, bam_view, bam_sort,
 * map_to_bam, extract_weak_reads, combine_genome_transcript and map_route calls, all through one function of the library --
 * is compressed on that device, one workgroup per block (csrc/ps_deflate.h: LZ77 with one candidate per hash, then stored,
 * fixed or dynamic Huffman by exact bit count).  The files are ordinary BAMs; block cuts, member headers, the end-of-file
 * block and the .bai arithmetic are the same, only the deflate payloads and their lengths differ from zlib's.  Returns
 * non-zero with the last error set when there is no such device.  A later HIP failure fails the writing call: there is no
 * fallback to zlib.  PS_BGZF_GPU=<device> in the environment is the same as the call; it is read once, when the library is
 * loaded, so the bwa, samtools and parasuite programs take it too.  PS_BAM_LEVEL means nothing on the device path (there is
 * one effort level).  PS_BGZF_PIECE: input bytes per launch (default 64 MiB, at least one block).
 * PS_BGZF_BTYPE=stored|fixed|dynamic restricts the encodings (tests; a block that would grow is stored all the same). */
int     ps_bgzf_device(int device);
/* src[0, n) cut at 0xff00 bytes as the file writers cut it -> the BGZF members in dst, without an end-of-file block, compressed
 * on `device` whatever the switch says; device -1: by the library's host path instead (zlib at PS_BAM_LEVEL, default 1, on 16
 * threads; n_stored / n_fixed / n_dynamic then count each member's first DEFLATE block, kernel_ms is 0) -- the reference that
 * tools/bgzf_time.py times the device against.  n == 0 writes nothing.  When the members need more than cap bytes the call fails and
 * writes nothing.  stats->struct_size must hold sizeof(ps_bgzf_stats); out_bytes is what was written; kernel_ms the kernels alone. */
typedef struct { uint32_t struct_size, n_blocks, n_stored, n_fixed, n_dynamic, pad_; uint64_t in_bytes, out_bytes; double kernel_ms; } ps_bgzf_stats;
int     ps_bgzf_compress(const void *src, uint64_t n, int device, void *dst, uint64_t cap, ps_bgzf_stats *stats /* may be NULL */);

/* ---- BAM records built on the device ------------------------------------------------------------------------------
 * ps_map_to_bam and every pass of ps_map_route / ps_map_route_opts turn a located piece into BAM records.  By default host
 * threads do that.  With the switch on (on != 0; PS_BAM_RECORDS_GPU=1 in the environment is the same, read once when the
 * library is loaded) the device that mapped the piece builds the record of every read it finished itself, right after the
 * locate stage and on the same stream: name, CIGAR, bases, qualities and the tags XT NM XN X0 X1 XM XO XG MD, byte for byte what
 * the host route writes (csrc/ps_bamrec.h states the record once for both).  Reads finished on the host (several best
 * intervals, XA lists, larger tiers) keep their records from the host route, spliced into the same stream.  The records, the
 * sorted files and their .bai are the same with the switch on or off; an unsorted file has one buffer of records per piece
 * instead of one per host thread, so its BGZF block cuts differ and its inflated bytes do not.  A HIP error fails the writing
 * call: there is no fallback to the host route.  ps_map, ps_map_profiled and ps_sam_to_bam are not touched by the switch.
 * ps_bam_records_info: counters summed over the process since the switch was last set (records by who built them, bytes, and
 * the route's four times in ms: inputs up, kernels, host-built records, stream down). */
typedef struct { uint64_t n_reads, n_records, n_device, n_host, bytes; double ms_upload, ms_kernels, ms_host_records, ms_download; } ps_bam_records_stats;
int     ps_bam_records_device(int on);
int     ps_bam_records_info(ps_bam_records_stats *out);
/* The staged form, after ps_batch_locate: the batch's records with MAPQ >= min_mapq, in input order, back to back in dst.
 * on_device 0: the host route on `threads` threads; 1: the device route (`threads` build the host-finished reads' records).
 * Returns the byte count, -1 on error.  dst NULL: the count alone.  When the records need more than cap bytes the call fails with
 * both numbers in the error and dst untouched.  origin (may be NULL, as many bytes as there are kept records): 0 where the device
 * built the record, 1 where the host did. */
int64_t ps_batch_bam_records(ps_batch *b, int min_mapq, int on_device, int threads, void *dst, uint64_t cap, uint8_t *origin /* may be NULL */, ps_bam_records_stats *stats /* may be NULL */);

/* ---- the coordinate sort of BAM records on the device ----------------------------------------------------------------
 * Every sorted BAM the library writes (ps_sam_to_bam and ps_map_to_bam with sort_by_coordinate, ps_bam_sort without by_name, the
 * sorted passes of ps_map_route / ps_map_route_opts, ps_combine_genome_transcript) orders its records with one stable sort on one
 * host thread and gathers them into the file's stream on host threads.  The device switch: -1 (the default) is that host route;
 * device >= 0 means that from now on the records' bytes go up to that device, a 64-bit key per record ((uint32_t)ref high,
 * pos ^ 0x80000000 low: unplaced records last, positions as signed numbers) is sorted there by a stable radix sort, a hand-written
 * kernel gathers the records into the sorted stream, and the permutation and the stream come down (csrc/ps_bamsort.h states the
 * key and the gather once for host and device).  Block cuts, compression, the file and the .bai are made as before, from the same
 * bytes: the files are the same with the switch on or off.  The name sort has a switch of its own (below).  The host route is taken, and counted
 * in n_calls_host, when there are 2^32 records or more or when the call would need more than PS_BAM_SORT_MAX_MB (default 32768)
 * of device memory.  Returns non-zero with the last error set when there is no such device.  A later HIP failure fails the writing
 * call: there is no fallback.  PS_BAM_SORT_GPU=<device> in the environment is the same as the call; it is read once, when the
 * library is loaded, so the bwa, samtools and parasuite programs take it too.  PS_BAM_SORT_PIECE: bytes of one half of the
 * page-locked staging that both sorts' records, columns, permutation and stream pass through (for tests: default 64 MiB and never
 * more, at least 256, rounded down to a multiple of 64; unset, empty, not a number or <= 0: the default); read at every call.
 * ps_bam_sort_info: summed over the process since the switch was last set; on_device: the switch is on; bytes: record bytes
 * sorted on the device; the route's four times in ms (records up, keys + sort, offsets + gather, permutation + stream down).
 * When ps_bgzf_device names the same device and the call keeps no records in memory (every call but the passes of ps_map_route
 * whose records go on to the next step), the sorted stream does not come down at all: the compressor reads it where it lies, and
 * only the permutation (for the .bai), the blocks' sizes, CRCs and packed images cross to the host.  n_resident counts these calls.
 * The file is the one that the BGZF switch alone writes, byte for byte. */
int     ps_bam_sort_device(int device);
typedef struct { uint32_t struct_size, on_device; uint64_t n_records, bytes, n_calls_device, n_calls_host, n_resident;
                 double ms_upload, ms_sort, ms_gather, ms_download; } ps_bam_sort_stats;
int     ps_bam_sort_info(ps_bam_sort_stats *out);
/* records: BAM records back to back, block_size first (what ps_batch_bam_records emits) -> the same records in coordinate order
 * in dst.  device >= 0: the device route whatever the switch says; -1: the library's host route (the stable sort and the gather
 * on `threads` threads), the reference that tools/bam_sort_time.py measures against.  Returns the byte count, -1 on error.  A
 * record that runs past n_bytes, or a block_size below 32, fails the call with the record's number.  When the records need more
 * than cap bytes the call fails and writes nothing; dst is untouched on any error.  n_bytes == 0 writes nothing and returns 0.
 * stats (struct_size must hold sizeof(ps_bam_sort_stats)): this call alone. */
int64_t ps_bam_sort_records(const void *records, uint64_t n_bytes, int device, int threads, void *dst, uint64_t cap, ps_bam_sort_stats *stats /* may be NULL */);

/* ---- the name sort of BAM records on the device ------------------------------------------------------------------------
 * Every name-sorted BAM the library writes (ps_bam_sort with by_name, `samtools sort -n` through the shim, the name-sorted
 * transcript pass of ps_map_route / ps_map_route_opts) orders its records with one stable sort on one host thread whose comparator
 * walks two names byte by byte, digit runs compared as numbers, then first of pair before second.  This switch is that sort's own:
 * ps_bam_sort_device and PS_BAM_SORT_GPU keep meaning the coordinate sort alone, and neither sort ever asks the other's switch.
 * device >= 0: the records go up as they do for the coordinate sort; a kernel writes a normalised key per name whose bytes order
 * exactly as the comparator does (csrc/ps_namesort.h states it once for host and device: a byte that is no digit as itself, a digit
 * run as 0x30, the length without leading zeros, the digits left; zero padding; the pair bits in the row's last byte), as a row of
 * key_words 32-bit words, column-major; from the last column to the first, a stable radix sort orders the records by one column --
 * columns in which all rows agree are skipped, n_passes counts the others; then the coordinate route's gather, download and -- when
 * ps_bgzf_device names the same device and the call keeps no records -- resident hand-over (n_resident).  The files are the same
 * with the switch on or off.  The host route is taken, and counted in n_calls_host, when there are 2^32 records or more, when a
 * record's name does not end inside the record, or when the call would need more than PS_BAM_SORT_MAX_MB of device memory (the
 * coordinate route's need and 4 * key_words bytes per record).  Returns non-zero with the last error set when there is no such
 * device.  A later HIP failure fails the writing call: there is no fallback.  -1 turns the route off, gives back its buffers (but
 * not those the coordinate switch still needs) and, like every setting, resets this switch's counters alone.
 * PS_BAM_NAME_SORT_GPU=<device> in the environment is the same as the call; it is read once, when the library is loaded.
 * ps_bam_name_sort_info: summed over the process since the switch was last set, key_words of the last device call; the route's
 * five times in ms (records up, the look at the names + rows, column sorts, offsets + gather, permutation + stream down). */
int     ps_bam_name_sort_device(int device);
typedef struct { uint32_t struct_size, on_device; uint64_t n_records, bytes, n_calls_device, n_calls_host, n_resident;
                 uint32_t key_words, pad_; uint64_t n_passes;
                 double ms_upload, ms_keys, ms_sort, ms_gather, ms_download; } ps_bam_name_sort_stats;
int     ps_bam_name_sort_info(ps_bam_name_sort_stats *out);
/* ps_bam_sort_records for the name order, with its contract: device >= 0 the device route whatever the switch says, -1 the
 * library's host route (the stable sort by the comparator and the pair bits, the gather on `threads` threads).  Beyond
 * ps_bam_sort_records' checks, a record whose name does not end inside it fails the call with the record's number. */
int64_t ps_bam_name_sort_records(const void *records, uint64_t n_bytes, int device, int threads, void *dst, uint64_t cap, ps_bam_name_sort_stats *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif
