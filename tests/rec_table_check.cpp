// rec_table_check.cpp -- stand-alone driver of csrc/ps_bam.cpp's record table and of csrc/ps_java.h for
// tests/test_rec_table_cpu.py (host compiler, sanitizers on, no device).
//   rec_table_check table <sam or bam> <column mask> <threads> <rows: i,j,.. or ->   the table, one line per record (below);
//                                                                                    an error: "error: <text>", exit status 2
//   rec_table_check double <decimal>...        Double.toString of each
//   rec_table_check float_div (<a> <b>)...     Float.toString of (float) a / (float) b
//   rec_table_check parse_int <text>...        Integer.parseInt of each: the value, or NumberFormatException
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ps_bam.h"
#include "ps_error.h"
#include "ps_java.h"

using namespace ps;

static void hex(const uint8_t *p, size_t n) { if (!n) std::printf("-"); for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]); }

// header: "n", "sort_order", "refs", "sizes <cigar words> <seq bytes> <qual bytes> <name bytes>", then per record
// "<ref> <pos> <flag> <l_seq> | <cig_off> <n_cig> <words,..> | <seq_off> <seq bytes hex> <qual bytes hex, padding included> | <name_off> <name_len> <name>"
// with "-" for an empty list and for a column that was not asked for
static int table(const char *path, unsigned columns, int threads, const char *rows_arg)
{
    std::vector<int32_t> rows;
    const bool all = !std::strcmp(rows_arg, "-");
    for (const char *p = rows_arg; !all && *p;) { char *e; rows.push_back((int32_t)std::strtol(p, &e, 10)); p = *e ? e + 1 : e; }
    RecTable t;
    try {
        BamFile f;
        load_records(path, threads, f);
        flatten_records(f, columns, all ? nullptr : &rows, threads, t);
    } catch (const std::exception &e) { std::printf("error: %s\n", e.what()); return 2; }
    std::printf("n %zu\nsort_order %s\nrefs", t.n(), t.sort_order.empty() ? "-" : t.sort_order.c_str());
    for (auto &r : t.refs) std::printf(" %s:%u", r.first.c_str(), r.second);
    std::printf("\nsizes %zu %zu %zu %zu\n", t.cigar.size(), t.seq.size(), t.qual.size(), t.names.size());
    if (t.ref.size() != t.n() || t.pos.size() != t.n() || t.l_seq.size() != t.n()) { std::printf("error: column lengths differ\n"); return 3; }
    for (size_t j = 0; j < t.n(); ++j) {
        const size_t l = (size_t)t.l_seq[j];
        std::printf("%d %d %u %d |", t.ref[j], t.pos[j], t.flag[j], t.l_seq[j]);
        if (columns & kRecCigar) {
            std::printf(" %u %u ", t.cig_off[j], t.n_cig[j]);
            if (!t.n_cig[j]) std::printf("-");
            for (uint32_t c = 0; c < t.n_cig[j]; ++c) std::printf("%s%u", c ? "," : "", t.cigar[t.cig_off[j] + c]);
        } else std::printf(" -");
        std::printf(" |");
        if (columns & (kRecSeq | kRecQual)) {
            std::printf(" %llu ", (unsigned long long)t.seq_off[j]);
            if (columns & kRecSeq) hex(t.seq.data() + t.seq_off[j] / 2, (l + 1) / 2); else std::printf("-");
            std::printf(" ");
            if (columns & kRecQual) hex(t.qual.data() + t.seq_off[j], (l + 1) / 2 * 2); else std::printf("-");
        } else std::printf(" -");
        std::printf(" |");
        if (columns & kRecNames) std::printf(" %llu %u %.*s", (unsigned long long)t.name_off[j], t.name_len[j], (int)t.name_len[j], (const char *)t.names.data() + t.name_off[j]);
        else std::printf(" -");
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 6 && !std::strcmp(argv[1], "table")) return table(argv[2], (unsigned)std::atoi(argv[3]), std::atoi(argv[4]), argv[5]);
    if (argc >= 2 && !std::strcmp(argv[1], "double")) {
        for (int i = 2; i < argc; ++i) std::printf("%s\n", java_double_to_string(std::strtod(argv[i], nullptr)).c_str());
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "float_div")) {
        for (int i = 2; i + 1 < argc; i += 2) std::printf("%s\n", java_float_to_string((float)std::atoi(argv[i]) / (float)std::atoi(argv[i + 1])).c_str());
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "parse_int")) {
        for (int i = 2; i < argc; ++i) {
            int32_t v = 0;
            if (java_parse_int((const uint8_t *)argv[i], (uint32_t)std::strlen(argv[i]), v)) std::printf("%d\n", v); else std::printf("NumberFormatException\n");
        }
        return 0;
    }
    std::fprintf(stderr, "usage: rec_table_check table|double|float_div|parse_int ...\n");
    return 1;
}
