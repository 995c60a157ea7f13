// ps_reads.h -- the reads of a job in host memory, and the FASTQ / FASTA parser that fills them (ps_reads.cpp; host only).
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <vector>
#include "ps_error.h"

namespace ps {

// std::vector without the zero fill of resize(): the parser's arrays (hundreds of MB per piece) are written once, by many threads
template <class T> struct DefaultInit : std::allocator<T> {
    template <class U> struct rebind { using other = DefaultInit<U>; };
    DefaultInit() noexcept {}
    template <class U> DefaultInit(const DefaultInit<U> &) noexcept {}
    template <class U> void construct(U *p) noexcept(std::is_nothrow_default_constructible<U>::value) { ::new (static_cast<void *>(p)) U; }
    template <class U, class... A> void construct(U *p, A &&...a) { ::new (static_cast<void *>(p)) U(std::forward<A>(a)...); }
};
template <class T> using RawVec = std::vector<T, DefaultInit<T>>;

struct ReadSet {
    int64_t n = 0;
    RawVec<int32_t> len;
    RawVec<int64_t> off;             // n+1 offsets into seq / qual
    RawVec<uint8_t> seq;             // codes 0..3, 4 = N, read orientation
    RawVec<char> qual; bool has_qual = false;
    RawVec<char> names; RawVec<int64_t> name_off;            // n+1
    const char *name(int64_t i, size_t &l) const { l = (size_t)(name_off[i + 1] - name_off[i]); return names.data() + name_off[i]; }
};
void load_reads(const char *path, ReadSet &rs, int threads = 1); // FASTQ or FASTA; plain, gzip or BGZF (ps_inflate.h)
// The input in pieces of whole records, in order; sink(piece) may block.  The file is STREAMED in windows of <= 64 MB (a compressed
// one inflated as it goes: its text has no known size, so the end of the input is met as on a FIFO); a piece is the
// windows parsed so far and goes out when another window would take it over chunk_bytes (first_bytes for the first piece, doubling from
// there) or -- `hungry` given -- as soon as it holds hungry_min_bytes and hungry() says that the stage behind is waiting for work.
void load_reads_chunked(const char *path, int threads, size_t chunk_bytes, const std::function<void(ReadSet &&)> &sink, size_t first_bytes = 0,
                        const std::function<bool()> *hungry = nullptr, size_t hungry_min_bytes = 0);
void reads_from_codes(int64_t n, int len, const uint8_t *codes, ReadSet &rs);
void parse_check(const char *reads_path, int threads, size_t chunk_bytes, uint64_t out[4]);   // ps_parse_check: {reads, bases, hash, pieces}

}  // namespace ps
