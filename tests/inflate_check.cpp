// inflate_check.cpp -- stand-alone driver of csrc/ps_inflate.cpp, the byte source of the text inputs, for
// tests/test_parser_gzip_cpu.py: built by the host compiler with AddressSanitizer and UBSan, run as a plain executable.
//   inflate_check read FILE             the file through the source with request sizes 1, 7, 4096 and 1 MiB (and on 1 and 4
//                                       threads): "<bytes> <FNV-1a hash>" when all agree; "error: ..." and exit status 3 when the
//                                       source throws (every request size must throw then)
//   inflate_check sweep FILE SEED N     N damaged copies of FILE in FILE.sweep, by turns one byte changed and the file cut short,
//                                       each read as above; one line per case: "<bytes> <hash>" or "error".  The first two bytes
//                                       stay: they are what says that the file is compressed at all, and a file without them
//                                       is a plain one whose bytes are delivered as they are
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "ps_inflate.h"

namespace {

struct Result { bool failed = false; std::string msg; uint64_t bytes = 0, hash = 0; };

Result read_through(const char *path, size_t request, int threads)
{
    Result r;
    try {
        ps::ByteSource src(path, "cannot open ", (size_t)256 << 10);
        std::vector<char> buf(request);
        uint64_t h = 1469598103934665603ull;
        for (;;) {
            const size_t got = src.read(buf.data(), request, threads);
            for (size_t i = 0; i < got; ++i) { h ^= (unsigned char)buf[i]; h *= 1099511628211ull; }
            r.bytes += got;
            if (got < request) break;
        }
        r.hash = h;
    } catch (const std::exception &e) { r.failed = true; r.msg = e.what(); }
    return r;
}

// all request sizes must tell the same story
Result read_every_way(const char *path)
{
    const size_t sizes[4] = {1, 7, 4096, (size_t)1 << 20};
    Result first;
    for (int k = 0; k < 4; ++k)
        for (int threads = 1; threads <= 4; threads += 3) {
            const Result r = read_through(path, sizes[k], threads);
            if (k == 0 && threads == 1) { first = r; continue; }
            if (r.failed != first.failed || r.bytes != (first.failed ? r.bytes : first.bytes) || (!r.failed && r.hash != first.hash)) {
                std::fprintf(stderr, "request size %zu on %d thread(s) disagrees with size 1: %s / %s\n", sizes[k], threads, r.msg.c_str(), first.msg.c_str());
                std::exit(4);
            }
        }
    return first;
}

std::vector<unsigned char> slurp(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    std::vector<unsigned char> d; unsigned char b[65536]; size_t n;
    while ((n = std::fread(b, 1, sizeof b, f)) > 0) d.insert(d.end(), b, b + n);
    std::fclose(f);
    return d;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "read")) {
        const Result r = read_every_way(argv[2]);
        if (r.failed) { std::printf("error: %s\n", r.msg.c_str()); return 3; }
        std::printf("%llu %llu\n", (unsigned long long)r.bytes, (unsigned long long)r.hash);
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "sweep")) {
        const std::vector<unsigned char> good = slurp(argv[2]);
        uint64_t s = std::strtoull(argv[3], nullptr, 10) * 2 + 1;
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
        const std::string tmp = std::string(argv[2]) + ".sweep";
        for (long c = 0, n = std::atol(argv[4]); c < n; ++c) {
            std::vector<unsigned char> d = good;
            const size_t at = 2 + (size_t)(rnd() % (good.size() - 2));
            if (c % 3 == 2) d.resize(at);                                    // cut short
            else d[at] = (unsigned char)(d[at] ^ (1 + rnd() % 255));         // one byte changed
            FILE *f = std::fopen(tmp.c_str(), "wb");
            if (!f || std::fwrite(d.data(), 1, d.size(), f) != d.size() || std::fclose(f)) { std::fprintf(stderr, "cannot write %s\n", tmp.c_str()); return 2; }
            const Result r = read_every_way(tmp.c_str());
            if (r.failed) std::printf("error\n"); else std::printf("%llu %llu\n", (unsigned long long)r.bytes, (unsigned long long)r.hash);
        }
        std::remove(tmp.c_str());
        return 0;
    }
    std::fprintf(stderr, "usage: inflate_check read FILE | sweep FILE SEED N\n");
    return 2;
}
