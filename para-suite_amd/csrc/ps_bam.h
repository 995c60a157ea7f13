// ps_bam.h -- SAM text -> BAM / sorted BAM + .bai, and the same operations on BAM input (host only, zlib).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "ps_outfiles.h"
namespace ps {
struct BamStats { uint64_t n_in = 0, n_out = 0, bam_bytes = 0; };
// Every BGZF block of every writer below is made by one batch function (ps_bam.cpp: bgzf_batch): spans of at most kBgzfBlock bytes ->
// comp[k], the whole gzip member of spans[k].  By default zlib on host threads.  A compressor registered here takes the whole
// list instead (the device compressor of ps_bgzf.hip; this file and ps_bam.cpp stay free of HIP); it throws ps::Error, and the
// writing call fails with it -- there is no fallback to zlib.  Null: zlib again.
struct BgzfSpan { const char *p; size_t n; };
const size_t kBgzfBlock = 0xff00;                 // the input bytes of one block, and where every writer cuts
inline void bgzf_cut(const char *p, size_t n, std::vector<BgzfSpan> &spans) { for (size_t a = 0; a < n; a += kBgzfBlock) spans.push_back(BgzfSpan{p + a, std::min(kBgzfBlock, n - a)}); }   // [p, p + n) in blocks, appended
typedef void (*BgzfBatchFn)(const BgzfSpan *spans, size_t n_spans, std::string *comp);
void bgzf_set_device_compressor(BgzfBatchFn fn);
void bgzf_host_compress(const BgzfSpan *spans, size_t n_spans, int level, int threads, std::string *comp);   // the host path itself, whatever is registered
// one member: the 16 fixed bytes with the BC field, BSIZE, the DEFLATE payload, CRC32 and ISIZE of the input -- for both compressors
void bgzf_member(const void *payload, size_t n_payload, uint32_t crc, uint32_t isize, std::string &out);
// THE BODY of a file: where the records' bytes are, in file order.  Still in the parts the records name (write_bam gathers them),
// one stream on the host, or one stream on a device.  The value owns what it names: a device stream goes back to where it came from
// when the body is destroyed, whether its blocks were made or not.
struct DeviceStream {                             // ps_bamsort.hip implements it; no HIP here
    virtual ~DeviceStream() {}
    virtual void blocks(std::string *comp) = 0;   // the BGZF members of the stream cut at kBgzfBlock bytes, comp[k] for block k; at most once
};
struct BamBody {
    std::string host; std::unique_ptr<DeviceStream> device; bool in_parts = true;   // in_parts: neither stream holds anything yet
    double ms_sort = -1; const char *route = "host";                                // of the sort that made it, for write_bam's stage line (PS_VERBOSE)
};
// The sort of every writer below (BamSink::finish, sam_to_bam, bam_sort) is one std::stable_sort on one thread; write_bam then gathers
// the records into the file's stream on host threads.  A hook registered here takes both instead (ps_bamsort.hip: the key, the
// radix sort and the gather on the device; this file and ps_bam.cpp stay free of HIP): it fills perm, the sorted order, and body:
// the records in that order back to back in body->host, or -- only when may_stay says that the caller can do without the stream on
// the host, and the BGZF switch names the hook's device -- in body->device.  It returns false when it leaves the call to the host
// route (and counts that; body is as it was), throws ps::Error on a device error -- the writing call fails with it, there is no
// fallback.  Null: the host route.  The name sort (`samtools sort -n`'s order, bam_name_cmp, then first of pair before second) has a
// hook of its own with the same contract: ps_bamsort.hip's name route, whose key ps_namesort.h states.  Each sort asks its own hook.
struct BamRec;
struct BamSortJob {
    const BgzfSpan *parts; size_t n_parts;        // the buffers the records lie in; recs[i].part names one
    const BamRec *recs; size_t n_recs;
    std::vector<uint32_t> *perm; BamBody *body; bool may_stay = false;
};
typedef bool (*BamSortFn)(BamSortJob &job);
void bam_sort_set_device_hook(BamSortFn fn);
void bam_name_sort_set_device_hook(BamSortFn fn);
// one encoded BAM record inside a buffer of records: reference id, 0-based position and end, flag, byte range [off, off + len)
struct BamRec { int32_t ref; int32_t pos; int32_t end; uint32_t flag; size_t off, len; int part; };
// The record layout (SAMv1 4.2), for every route that makes records -- SAM text (sam_to_bam) and the mapper's hits (ps_map_to_bam).
// In this order: begin, CIGAR words, the caller's (l_seq + 1) / 2 bytes of base nibbles and l_seq bytes of Phred values, tags, end.
struct BamCore { int32_t ref, pos; int64_t end; int mapq, flag; uint32_t n_cigar, l_seq; int32_t rnext = -1, pnext = -1, tlen = 0; };   // pos, pnext 0-based; end: pos + reference bases covered (at least 1)
void bam_rec_begin(std::string &o, const BamCore &c, const char *name, size_t name_len, BamRec &r);   // fixed part (bin from pos / end) + name; r: all but len and part
void bam_rec_cigar(std::string &o, const uint32_t *words, size_t n);
void bam_tag_int(std::string &o, const char *tag, long long v);                                       // the smallest type that holds v, as htslib's SAM parser
void bam_tag_char(std::string &o, const char *tag, char v);                                           // type A
void bam_tag_text(std::string &o, const char *tag, char type /* Z or H */, const char *v, size_t n);
void bam_tag_text_open(std::string &o, const char *tag, char type);                                  // the same tag with a value the caller appends to o itself,
void bam_tag_text_close(std::string &o);                                                              // then closes
void bam_rec_end(std::string &o, BamRec &r);                                                          // block_size and r.len
// BAM records that were never SAM text (ps_map_to_bam: straight from the alignment records in memory): parts arrive in input
// order.  Unsorted output: a part is cut into BGZF blocks, compressed on `threads` threads and appended to the file at once, so the
// compression of one piece of the input runs while the next is searched.  Coordinate-sorted output (+ .bai): the parts are kept and
// sorted, compressed and written by finish().  sort_by_name: the same with the names ordered as `samtools sort -n` orders them
// (ps_bam_sort's rule) under @HD SO:queryname.  finish(.., keep): the records of the sorted file stay in memory, in file order, as
// load_records() would return them -- the file's stream as the one part (ps_map_route hands them to the lift instead of reading the file back).
struct BamFile;
class BamSink {
public:
    BamSink(const std::string &header_text, const std::vector<std::pair<std::string, uint32_t>> &refs, const char *bam_path,
            bool sort_by_coordinate, bool write_index, int threads, int level, bool sort_by_name = false);
    ~BamSink();
    // buffers of records in input order (one per encoding thread); recs[k][i].off/len index into records[k]; both are consumed
    void add(std::vector<std::string> &records, std::vector<std::vector<BamRec>> &recs, uint64_t n_in);
    // one buffer of records that stays the caller's (the device route's page-locked download: ps_bamrec.hip); recs[i].off / len index into it.
    // Unsorted output is cut and compressed straight from the span -- one buffer, so a block never spans two; a sorted sink, which has to
    // keep the records until finish(), takes its copy.  recs is consumed.
    void add(const char *records, size_t n_bytes, std::vector<BamRec> &recs, uint64_t n_in);
    void finish(BamStats *stats, BamFile *keep = nullptr);
private:
    struct Impl; Impl *p;
};
// a BAM among a call's outputs, with the <path>.bai that BamSink and the writers below put beside the path they are given
inline std::string add_bam(OutFiles &files, const std::string &bam, bool index) { const std::string t = files.add(bam); if (index) files.add(bam + ".bai", t + ".bai"); return t; }
// all throw ps::Error; each owns its outputs (ps_outfiles.h) and refuses one that is its input.  min_mapq: records with MAPQ below it are dropped (samtools view -q)
void sam_to_bam(const char *sam_path, const char *bam_path, int min_mapq, bool sort_by_coordinate, bool write_index, int threads, BamStats *stats);
void bam_view(const char *in_bam, const char *out_bam, int min_mapq, int threads, BamStats *stats);     // samtools view -q Q -b
void bam_sort(const char *in_bam, const char *out_bam, bool by_name, int threads, BamStats *stats);    // samtools sort [-n]
void bam_index(const char *bam, int threads);                                                           // samtools index -> <bam>.bai
// the records of a SAM or BAM file as they are encoded (SAMv1 4.2), for the steps that pass records on: name, MAPQ, mate fields,
// QUAL and the raw tag bytes are all in rec(i); recs[i] carries reference id, position, end and flag.  Records in file order;
// the records of part k are one run of recs, parts in order.
struct BamFile {
    std::string text; std::vector<std::pair<std::string, uint32_t>> refs;   // header text, @SQ name and length
    std::vector<std::string> enc; std::vector<BamRec> recs;
    std::string sort_order;                                                 // SO: of the @HD line ("" when there is none)
    size_t n() const { return recs.size(); }
    const uint8_t *rec(size_t i) const { return (const uint8_t *)enc[(size_t)recs[i].part].data() + recs[i].off; }   // block_size first
};
void load_records(const char *sam_or_bam, int threads, BamFile &out);
// BAM records back to back, block_size first -> one BamRec each (ref, pos, off, len; part 0).  A record that runs past n_bytes or a
// block_size below 32 throws with the record's number (1-based).
void scan_records(const char *records, uint64_t n_bytes, std::vector<BamRec> &recs);
// the host route on its own: recs into coordinate order (std::stable_sort), their bytes gathered into dst on `threads` threads
void sort_records_host(const char *records, std::vector<BamRec> &recs, int threads, char *dst);
// the name order's comparator (read names as `samtools sort -n` orders them: digit runs compare as numbers; NUL-terminated), and the
// host route of that order: recs (every name ends inside its record) by bam_name_cmp, then the pair bits of the flag, then gathered
int bam_name_cmp(const char *a, const char *b);
// l_read_name (byte 12 of a record, block_size first) counts the NUL that ends the name at byte 36 + l_read_name - 1
inline bool name_ends_inside(const uint8_t *rec, size_t len) { return len >= 37 && rec[12] >= 1 && 36 + (size_t)rec[12] <= len && rec[36 + rec[12] - 1] == 0; }
void sort_records_host_by_name(const char *records, std::vector<BamRec> &recs, int threads, char *dst);
// The record table: the fields of the records of a BamFile as flat arrays, for the analysis modes' kernels.
// ref, pos, flag and l_seq always; the other columns by mask.  BAM conventions throughout: pos 0-based (a kernel that wants
// htsjdk's 1-based start adds one), ref -1 unplaced, CIGAR words len<<4|op with MIDNSHP=X, bases as nibbles =ACMGRSVTWYHKDBN.
enum : unsigned { kRecCigar = 1, kRecSeq = 2, kRecQual = 4, kRecNames = 8 };
struct RecTable {
    unsigned columns = 0;
    std::vector<std::pair<std::string, uint32_t>> refs; std::string sort_order;   // as the BamFile has them
    std::vector<int32_t> ref, pos, l_seq; std::vector<uint32_t> flag;
    std::vector<uint32_t> cig_off, n_cig, cigar;               // kRecCigar
    std::vector<uint64_t> seq_off;                             // kRecSeq or kRecQual: in bases and always even (records start on a byte)
    std::vector<uint8_t> seq;                                  // kRecSeq: base j of a record is nibble (seq_off + j)
    std::vector<uint8_t> qual;                                 // kRecQual: Phred value of base j at byte (seq_off + j); QUAL absent: 0xFF, as a record's padding byte
    std::vector<uint64_t> name_off; std::vector<uint8_t> name_len, names;   // kRecNames: the name's bytes without its NUL
    size_t n() const { return flag.size(); }
};
// rows: the records to take, in this order (null: all).  The fill runs on `threads` threads.  Every record is checked against its own
// length first: "corrupt record N", "record N refers to a reference that is not in the header" (N: 1-based, in the file), and
// "more than 2^32 CIGAR operations" -- the caller puts its name in front.
void flatten_records(const BamFile &f, unsigned columns, const std::vector<int32_t> *rows, int threads, RecTable &out);
void load_rec_table(const char *sam_or_bam, unsigned columns, int threads, RecTable &out);   // load_records + flatten_records of all rows
struct ExtractStats { uint64_t n_records = 0, n_weak = 0, n_kept = 0, bam_bytes = 0; };
// ExtractWeakMappingReads.extractReads: records with MAPQ < mapq_threshold -> four FASTQ lines each (read orientation restored),
// the others -> out_bam with the input's header
void extract_weak_reads(const char *sam_or_bam, const char *out_bam, const char *out_fastq, int mapq_threshold, int threads, ExtractStats *stats);
struct NamesStats { uint64_t n_records = 0, out_bytes = 0; };
// ExtractNotMappedReads.extractReads: "@" + QNAME + "\n" per record, in file order
void extract_read_names(const char *sam_or_bam, const char *out_file, int threads, NamesStats *stats);
}
