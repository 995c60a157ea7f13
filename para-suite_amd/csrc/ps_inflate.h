// ps_inflate.h -- one byte source for the text inputs (FASTQ / FASTA): plain, gzip (RFC 1952) or BGZF, told apart by the input's
// first two bytes (ps_inflate.cpp; host only, zlib, nothing from HIP -- tests/inflate_check.cpp builds the pair alone).
//
// Upstream `bwa` opens every input through zlib's gzopen, so `reads.fastq.gz` and `genome.fa.gz` are accepted wherever
// PARAsuiteMapping.java:73-74 and BWAMapping.java hand it a path.  The same here: concatenated members are decoded one after the
// other, empty members yield nothing, an input that does not start with 1f 8b is passed through as it is.
// Deviations: (1) gzread hands out a truncated stream as if it ended there (bwa maps half a file and exits 0); here an input that
// ends inside a member -- in its header, its data or its trailer -- is an error.  (2) gzread ignores bytes behind the last member;
// here bytes behind a complete member that do not start another member are an error: a file that was damaged or glued together
// wrongly is named, not half-read.
//
// No device work: one DEFLATE stream is a serial chain (every symbol's bit position and the 32 KB window depend on all before
// it), and BGZF's independent blocks feed a parser that runs on the host.
// This speaks of inflating.  Compressing has no such chain across BGZF blocks, and the blocks a BAM writer makes can be compressed
// on the device (ps_deflate.h, ps_bgzf.hip).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <zlib.h>
#include <sys/types.h>
#include "ps_error.h"

namespace ps {

// ---- the two pieces that exist once: ps_bam.cpp's BAM reader and the BGZF kind of the source below share them (inline, so that
// ps_bam.cpp still builds alone, as tests/rec_table_check.cpp builds it)
const size_t kBgzfMaxOut = 65536;                                 // SAMv1 4.1: a block holds at most 64 KiB, compressed and not
inline uint32_t le16(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const unsigned char *p) { return le16(p) | (le16(p + 2) << 16); }

// The gzip member header at p[0, n).  1: a well-formed header of `len` bytes; `bsize` is the whole BGZF block's size (BSIZE + 1)
// when the extra field holds the BC subfield, else 0.  0: p[0, n) ends inside the header (give more bytes, or the input is cut
// there).  -1: not a header this library reads; `why` says what (static text).
inline int gz_member_header(const unsigned char *p, size_t n, size_t &len, size_t &bsize, const char *&why)
{
    len = 0; bsize = 0; why = nullptr;
    if ((n >= 1 && p[0] != 31) || (n >= 2 && p[1] != 139)) { why = "not a gzip member"; return -1; }
    if (n >= 3 && p[2] != 8) { why = "compression method other than 8 (deflate)"; return -1; }
    if (n >= 4 && (p[3] & 0xe0)) { why = "reserved flag bits set in a member header"; return -1; }
    if (n < 10) return 0;
    const int flg = p[3];
    size_t at = 10;
    if (flg & 4) {                                           // FEXTRA: subfields SI1 SI2 LEN data
        if (n < at + 2) return 0;
        const size_t xlen = le16(p + at);
        if (n < at + 2 + xlen) return 0;
        for (size_t q = at + 2, e = at + 2 + xlen; q + 4 <= e;) {
            const size_t sl = le16(p + q + 2);
            if (q + 4 + sl > e) break;
            if (p[q] == 'B' && p[q + 1] == 'C' && sl == 2) { bsize = (size_t)le16(p + q + 4) + 1; break; }
            q += 4 + sl;
        }
        at += 2 + xlen;
    }
    for (int f = 8; f <= 16; f <<= 1)                        // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            const void *z = at < n ? std::memchr(p + at, 0, n - at) : nullptr;
            if (!z) return 0;
            at = (size_t)((const unsigned char *)z - p) + 1;
        }
    if (flg & 2) {                                           // FHCRC: the low 16 bits of the header's CRC32
        if (n < at + 2) return 0;
        if ((crc32(crc32(0L, Z_NULL, 0), p, (uInt)at) & 0xffffu) != le16(p + at)) { why = "header CRC16 mismatch"; return -1; }
        at += 2;
    }
    len = at;
    return 1;
}

// One BGZF block block[0, bsize) whose header is head_len bytes: its ISIZE word, and the inflate of its data into exactly that many
// bytes at dst with the CRC32 checked: nullptr, or static text that says what is wrong.
inline uint32_t bgzf_isize(const unsigned char *block, size_t bsize) { return le32(block + bsize - 4); }
inline const char *bgzf_inflate_block(const unsigned char *block, size_t bsize, size_t head_len, char *dst, uint32_t isize)
{
    if (bsize < head_len + 8) return "BSIZE too small for a block";
    unsigned char none = 0;                                  // an empty block still decodes its end-of-block symbol
    z_stream zs; std::memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return "inflateInit2 failed";
    zs.next_in = const_cast<unsigned char *>(block) + head_len; zs.avail_in = (uInt)(bsize - head_len - 8);
    zs.next_out = isize ? (Bytef *)dst : &none; zs.avail_out = isize ? isize : 1;
    const int rc = inflate(&zs, Z_FINISH);
    const size_t made = zs.total_out, left = zs.avail_in;
    inflateEnd(&zs);
    if (rc == Z_BUF_ERROR && made == (isize ? isize : 1)) return "ISIZE mismatch";       // more data than the trailer states
    if (rc != Z_STREAM_END) return "invalid deflate data";
    if (made != isize) return "ISIZE mismatch";
    if (left) return "invalid deflate data";                 // the deflate stream ends in front of the trailer
    if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)(isize ? (unsigned char *)dst : &none), isize) != le32(block + bsize - 8)) return "CRC32 mismatch";
    return nullptr;
}

// ---- the source
// The input's bytes in order.  read(dst, want, threads) returns the bytes delivered; fewer than `want`: the input ends there.
//   plain  regular files by parallel pread on up to 8 of `threads`, other inputs (FIFOs) by read; the size is known for regular files
//   gzip   one inflater thread runs ahead of the reader through a bounded hand-over of at most two windows of `window` bytes
//   BGZF   (first member carries BC) the blocks of one read() are inflated side by side on `threads`, straight into dst; a later
//          member without BC hands the rest of the stream to the serial decoder
// Every error is a ps::Error that names the file and, for compressed input, the compressed byte offset.  No thread outlives the
// object: the inflater is joined in the destructor, whether the stream failed, ended or was left half-read.
class ByteSource {
public:
    // open_error: what goes in front of the path when it cannot be opened ("cannot open reads ")
    ByteSource(const char *path, const char *open_error, size_t window = (size_t)64 << 20);
    ~ByteSource();
    ByteSource(const ByteSource &) = delete;
    ByteSource &operator=(const ByteSource &) = delete;
    size_t read(char *dst, size_t want, int threads);
    bool size_known() const;                 // plain regular files only: a compressed input's text has no known size
    uint64_t size() const;                   // of the text, when known
    bool compressed() const;
private:
    struct Impl; Impl *p;
};

// the whole input into out (a std::vector<char> or std::string), which ends up exactly as long as the text
template <class V> void read_all(ByteSource &src, V &out, int threads)
{
    size_t have = 0, cap = src.size_known() ? (size_t)src.size() + 1 : (size_t)1 << 20;      // one byte over: a file of the size stated ends in one call
    for (;;) {
        out.resize(cap);
        const size_t got = src.read(&out[have], cap - have, threads);
        have += got;
        if (have < cap) break;
        cap *= 2;
    }
    out.resize(have);
}

// a regular file that starts with the gzip magic 1f 8b (what it holds has no known size); anything else, unreadable included: false
bool is_gzip_file(const char *path);

}  // namespace ps
