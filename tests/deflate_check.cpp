// deflate_check -- the host build of csrc/ps_deflate.h as a plain program (tests/test_deflate_cpu.py builds it with AddressSanitizer
// and UBSan): deflate_check IN OUT [stored|fixed|dynamic|all] cuts IN at 0xff00 bytes, encodes every block with the lanes run one
// after the other and writes the BGZF members (no end-of-file block) to OUT; per block one line on stdout: BTYPE, bytes of the
// stream, and the depth of the plain Huffman trees before the limit (literal/length, distance, code lengths).
// deflate_check lengths MAXBITS F0 F1 ...: the code lengths the encoder's tree builder gives symbols of these frequencies, then
// the depth of the plain tree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "ps_deflate.h"

int main(int argc, char **argv)
{
    if (argc > 3 && std::string(argv[1]) == "lengths") {
        std::unique_ptr<ps::DfShared> sh(new ps::DfShared);
        const int maxbits = std::atoi(argv[2]), nsym = argc - 3;
        if (nsym < 2 || nsym > 286 || maxbits < 1 || maxbits > 15) return 2;
        std::vector<uint32_t> f(288, 0); std::vector<uint8_t> len(288, 0);
        for (int k = 0; k < nsym; ++k) f[(size_t)k] = (uint32_t)std::strtoul(argv[3 + k], nullptr, 10);
        ps::df_build(*sh, f.data(), nsym, maxbits, len.data(), 0);
        for (int k = 0; k < nsym; ++k) std::printf("%u ", len[(size_t)k]);
        std::printf("\n%u\n", sh->max_depth[0]);
        return 0;
    }
    if (argc < 3) { std::fprintf(stderr, "usage: deflate_check IN OUT [stored|fixed|dynamic|all]\n"); return 2; }
    const std::string mode = argc > 3 ? argv[3] : "all";
    const uint32_t allow = mode == "stored" ? ps::DF_STORED : mode == "fixed" ? ps::DF_FIXED : mode == "dynamic" ? ps::DF_DYNAMIC : ps::DF_ALL;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<uint8_t> in;
    { uint8_t buf[65536]; size_t g; while ((g = std::fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + g); }
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    std::unique_ptr<ps::DfShared> sh(new ps::DfShared);
    for (size_t at = 0; at < in.size(); at += ps::DF_BLOCK) {
        const uint32_t n = (uint32_t)std::min<size_t>(ps::DF_BLOCK, in.size() - at);
        // exactly the bytes the encoder may touch: the sanitizer sees one byte more
        std::vector<uint8_t> src(in.begin() + (long)at, in.begin() + (long)(at + n));
        std::vector<uint32_t> out((n + 5 + 3) / 4), tok(n);
        ps::DfResult r{};
        ps::df_block(*sh, src.data(), n, out.data(), tok.data(), allow, &r);
        if (r.bytes > n + 5) { std::fprintf(stderr, "block of %u bytes grew to %u\n", n, r.bytes); return 1; }
        const uint32_t total = 18 + r.bytes + 8;
        uint8_t head[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, (uint8_t)((total - 1) & 0xff), (uint8_t)((total - 1) >> 8)};
        uint8_t tail[8];
        for (int k = 0; k < 4; ++k) { tail[k] = (uint8_t)(r.crc >> (8 * k)); tail[4 + k] = (uint8_t)(n >> (8 * k)); }
        std::fwrite(head, 1, 18, o); std::fwrite(out.data(), 1, r.bytes, o); std::fwrite(tail, 1, 8, o);
        std::printf("%u %u %u %u %u\n", r.btype, r.bytes, r.depth[0], r.depth[1], r.depth[2]);
    }
    if (std::fclose(o) != 0) { std::perror(argv[2]); return 2; }
    return 0;
}
