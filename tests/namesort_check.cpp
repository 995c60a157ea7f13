// namesort_check.cpp -- csrc/ps_namesort.h under the host compiler alone (tests/test_namesort_cpu.py builds it with AddressSanitizer
// and UBSan, together with csrc/ps_bam.cpp, and runs it as a plain program).  The reference of every comparison is the library's own
// comparator, bam_name_cmp (ps_bam.cpp's strnum_cmp).
//   exhaustive  every name of up to four bytes over {'0', '1', '9', 'a', '/', ':'} against every other: the sign of the comparison of
//               the two rows (pair byte zero) is the sign of bam_name_cmp.
//   random      1,000,000 pairs of names of 0 to 254 bytes, a share of them grown from a common prefix, with runs of 40 digits and
//               bytes at 0x80 and above; the pair byte decides between equal names.
//   length      a key is at most 2 * len + 1 bytes long, "1a1a...1" reaches that for every odd length up to 253 (an even one falls
//               one short), and after the key's end the generator hands out zeros alone.
//   order       a stable sort of 3,000 records by their rows is sort_records_host_by_name's order, and (swap) that order with two
//               records exchanged is not: the negative control.
// Rows and names live on heap buffers of the exact size.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ps_bam.h"
#include "ps_namesort.h"

using namespace ps;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }
static int fail(const char *what, const std::string &a = "", const std::string &b = "")
{
    std::fprintf(stderr, "FAIL %s", what);
    for (const std::string *s : {&a, &b}) { std::fprintf(stderr, " ["); for (unsigned char c : *s) std::fprintf(stderr, c >= 0x21 && c < 0x7f ? "%c" : "\\x%02x", c); std::fprintf(stderr, "]"); }
    std::fprintf(stderr, "\n");
    return 1;
}
static int sign(int v) { return v < 0 ? -1 : v > 0 ? 1 : 0; }

// a row on a heap buffer of exactly W words, made from a copy of the name of exactly its length (no NUL behind it)
struct Row {
    uint32_t *w; uint32_t W;
    Row(const std::string &name, uint32_t pair, uint32_t W_) : w((uint32_t *)std::malloc(4 * (size_t)W_)), W(W_)
    {
        uint8_t *exact = (uint8_t *)std::malloc(name.size() ? name.size() : 1);
        std::memcpy(exact, name.data(), name.size());
        namesort_row(exact, (uint32_t)name.size(), pair, W, w, 1);
        std::free(exact);
    }
    Row(const Row &) = delete;
    ~Row() { std::free(w); }
};

static bool rows_agree(const std::string &a, const std::string &b, uint32_t W)
{
    Row ra(a, 0, W), rb(b, 0, W);
    return sign(namesort_row_cmp(ra.w, rb.w, W, 1)) == sign(bam_name_cmp(a.c_str(), b.c_str()));
}

static int check_exhaustive()
{
    const char alphabet[] = {'0', '1', '9', 'a', '/', ':'};
    std::vector<std::string> names(1, "");
    for (size_t from = 0, len = 1; len <= 4; ++len) {
        const size_t to = names.size();
        for (size_t k = from; k < to; ++k) for (char c : alphabet) names.push_back(names[k] + c);
        from = to;
    }
    if (names.size() != 1555) return fail("exhaustive: the number of names");
    const uint32_t W = namesort_words(4);
    std::vector<uint32_t> rows(names.size() * W);
    for (size_t k = 0; k < names.size(); ++k) { Row r(names[k], 0, W); std::memcpy(&rows[k * W], r.w, 4 * (size_t)W); }
    size_t n_equal = 0;
    for (size_t x = 0; x < names.size(); ++x)
        for (size_t y = 0; y < names.size(); ++y) {
            const int want = sign(bam_name_cmp(names[x].c_str(), names[y].c_str()));
            if (sign(namesort_row_cmp(&rows[x * W], &rows[y * W], W, 1)) != want) return fail("exhaustive: rows and comparator disagree", names[x], names[y]);
            n_equal += want == 0;
        }
    if (!rows_agree("a0", "a00", 2) || bam_name_cmp("a0", "a00") != 0 || bam_name_cmp("r9", "r10") >= 0) return fail("exhaustive: the examples");
    std::printf("exhaustive ok: %zu names, %zu ordered pairs, %zu of them equal\n", names.size(), names.size() * names.size(), n_equal);
    return 0;
}

// names as read names come and as they should not: digits and separators next to each other, long numbers, high bytes
static std::string random_name(uint32_t max_len)
{
    static const unsigned char pool[] = {'0', '0', '1', '2', '5', '9', '/', '.', ':', '-', '_', 'a', 'b', 'Z', 0x7f, 0x80, 0xc3, 0xff};
    std::string s;
    const uint32_t len = below(4) == 0 ? below(max_len + 1) : below(std::min<uint32_t>(max_len, 24) + 1);
    while (s.size() < len) {
        const uint32_t kind = below(12);
        if (kind == 0) { for (int k = 0; k < 40 && s.size() < len; ++k) s.push_back((char)('0' + below(10))); }          // past 64 bits
        else if (kind == 1) { const uint32_t z = 1 + below(5); for (uint32_t k = 0; k < z && s.size() < len; ++k) s.push_back('0'); }
        else if (kind == 2) s.push_back((char)(1 + below(255)));
        else s.push_back((char)pool[below(sizeof pool)]);
    }
    return s;
}

static int check_random()
{
    const uint32_t W = namesort_words(NS_MAX_NAME);
    size_t n_prefix = 0, n_equal = 0, n_long_run = 0, n_high = 0;
    for (int k = 0; k < 1000000; ++k) {
        std::string a = random_name(NS_MAX_NAME), b;
        if (below(3) == 0) {                                                    // a common prefix, then a few bytes of its own
            b = a.substr(0, below((uint32_t)a.size() + 1));
            if (below(4)) b += random_name(std::min<uint32_t>(8, NS_MAX_NAME - (uint32_t)b.size()));
            ++n_prefix;
        } else b = random_name(NS_MAX_NAME);
        if (below(50) == 0 && a.size() >= 41) { b = a; b[40] = (char)(b[40] == '7' ? '8' : '7'); }   // differ in one late byte
        Row ra(a, below(4), W), rb(b, below(4), W);
        const int want = sign(bam_name_cmp(a.c_str(), b.c_str()));
        const int pa = (int)(ra.w[W - 1] & 0xff), pb = (int)(rb.w[W - 1] & 0xff);
        const int got = sign(namesort_row_cmp(ra.w, rb.w, W, 1));
        if (got != (want ? want : sign(pa - pb))) return fail("random: rows and comparator disagree", a, b);
        if (!rows_agree(a, b, namesort_words((uint32_t)std::max(a.size(), b.size())))) return fail("random: the narrowest row that holds both", a, b);
        n_equal += want == 0;
        for (const std::string *s : {&a, &b}) {
            uint32_t run = 0, longest = 0; bool high = false;
            for (unsigned char c : *s) { run = namesort_digit(c) ? run + 1 : 0; longest = std::max(longest, run); high |= c >= 0x80; }
            n_long_run += longest >= 40; n_high += high;
        }
    }
    if (n_prefix < 300000 || n_equal < 1000 || n_long_run < 10000 || n_high < 100000) return fail("random: the pairs do not cover what they should");
    std::printf("random ok: 1000000 pairs, %zu from a common prefix, %zu equal, %zu names with a run of 40 digits, %zu with bytes at 0x80 and above\n", n_prefix, n_equal, n_long_run, n_high);
    return 0;
}

// the key's bytes, by the generator alone, on an exact copy of the name; `more` further calls must all give zero
static bool key_of(const std::string &name, std::string &key, int more)
{
    uint8_t *exact = (uint8_t *)std::malloc(name.size() ? name.size() : 1);
    std::memcpy(exact, name.data(), name.size());
    NsGen g; key.clear();
    std::string all;
    for (size_t k = 0; k < 2 * name.size() + 1 + (size_t)more; ++k) all.push_back((char)namesort_next(g, exact, (uint32_t)name.size()));
    std::free(exact);
    size_t end = all.size();
    while (end > 0 && all[end - 1] == 0) --end;
    // an all-zero run at the very end of a name ends the key with its length byte, which is zero: the marker before it is the last byte
    key = all.substr(0, end);
    return end <= 2 * name.size() + 1;
}

static int check_length()
{
    std::string key;
    size_t n_full = 0;
    for (uint32_t len = 1; len <= NS_MAX_NAME; ++len) {
        std::string worst;
        for (uint32_t k = 0; k < len; ++k) worst.push_back(k & 1 ? 'a' : '1');
        if (!key_of(worst, key, 64)) return fail("length: a key longer than 2 * len + 1", worst);
        const size_t want = len & 1 ? 2 * (size_t)len + 1 : 2 * (size_t)len;      // (len + 1) / 2 runs of three bytes, len / 2 letters
        if (key.size() != want) return fail("length: the key of 1a1a...", worst);
        n_full += key.size() == 2 * (size_t)len + 1;
        if (4 * (size_t)namesort_words(len) < 2 * (size_t)len + 3 || 4 * (size_t)namesort_words(len) > 2 * (size_t)len + 6) return fail("length: the row's width");
    }
    if (namesort_words(0) != 1 || namesort_words(254) != 128 || namesort_words(1) != 2) return fail("length: the row's width at the ends");
    for (int k = 0; k < 20000; ++k) {
        const std::string s = random_name(NS_MAX_NAME);
        if (!key_of(s, key, 16)) return fail("length: a key longer than 2 * len + 1", s);
    }
    if (!key_of("a007", key, 8) || key != std::string("a\x30\x01" "7")) return fail("length: the key of a007");
    if (!key_of("x000", key, 8) || key != std::string("x\x30")) return fail("length: the key of x000");
    if (!key_of("", key, 8) || !key.empty()) return fail("length: the empty name");
    if (namesort_begin_bit(0x00ff0100u) != 8 || namesort_end_bit(0x00ff0100u) != 24 || namesort_begin_bit(0x80000000u) != 31 || namesort_end_bit(1u) != 1 || namesort_end_bit(0xffffffffu) != 32)
        return fail("length: the bit range of a column");
    std::printf("length ok: at most 2 * len + 1 bytes for every length to %d, reached by %zu names, zeros alone after the end\n", (int)NS_MAX_NAME, n_full);
    return 0;
}

// BAM records as far as the sort reads them: block_size, l_read_name at 12, the flag at 18, the name at 36
static void put_record(std::string &o, const std::string &name, uint32_t flag, uint32_t extra)
{
    const uint32_t len = 36 + (uint32_t)name.size() + 1 + extra, bs = len - 4;
    const size_t at = o.size();
    o.resize(at + len);
    for (uint32_t k = 4; k < len; ++k) o[at + k] = (char)rnd();
    for (int k = 0; k < 4; ++k) o[at + k] = (char)(bs >> (8 * k));
    o[at + 12] = (char)(name.size() + 1); o[at + 18] = (char)(flag & 0xff); o[at + 19] = (char)(flag >> 8);
    std::memcpy(&o[at + 36], name.data(), name.size()); o[at + 36 + name.size()] = 0;
}

static int check_order()
{
    const size_t N = 3000;
    std::string bytes; std::vector<std::string> names(N); std::vector<uint32_t> flags(N);
    for (size_t i = 0; i < N; ++i) {
        names[i] = below(3) == 0 && i ? names[below((uint32_t)i)] : "r" + random_name(12);          // many equal names
        if (below(5) == 0) names[i] = "r" + std::string(below(3), '0') + std::to_string(below(30));  // r7, r07, r007
        flags[i] = (below(4) << 6) | below(64) | (below(2) << 10);
        put_record(bytes, names[i], flags[i], below(40));
    }
    std::vector<BamRec> recs;
    scan_records(bytes.data(), bytes.size(), recs);
    if (recs.size() != N) return fail("order: the records");
    for (size_t i = 0; i < N; ++i) if (recs[i].flag != flags[i]) return fail("order: the flag of a record");
    uint32_t longest = 0;
    for (const std::string &s : names) longest = std::max<uint32_t>(longest, (uint32_t)s.size());
    const uint32_t W = namesort_words(longest);
    uint32_t *col = (uint32_t *)std::malloc(4 * (size_t)W * N);                                     // column-major, as the device keeps it
    for (size_t i = 0; i < N; ++i) {
        uint8_t *exact = (uint8_t *)std::malloc(names[i].size());
        std::memcpy(exact, names[i].data(), names[i].size());
        namesort_row(exact, (uint32_t)names[i].size(), namesort_pair(flags[i]), W, col + i, N);
        std::free(exact);
    }
    std::vector<uint32_t> by_rows(N);
    for (size_t i = 0; i < N; ++i) by_rows[i] = (uint32_t)i;
    // least significant column first, a stable sort per column: the passes of the device route
    for (uint32_t w = W; w-- > 0;) std::stable_sort(by_rows.begin(), by_rows.end(), [&](uint32_t x, uint32_t y) { return col[(size_t)w * N + x] < col[(size_t)w * N + y]; });
    std::vector<BamRec> sorted = recs;
    std::vector<char> dst(bytes.size());
    sort_records_host_by_name(bytes.data(), sorted, 3, dst.data());
    auto index_of = [&](const BamRec &r) { return (size_t)(std::lower_bound(recs.begin(), recs.end(), r, [](const BamRec &x, const BamRec &y) { return x.off < y.off; }) - recs.begin()); };
    auto same = [&](const std::vector<uint32_t> &order) { for (size_t k = 0; k < N; ++k) if (index_of(sorted[k]) != order[k]) return false; return true; };
    const bool good = same(by_rows);
    std::free(col);
    if (!good) return fail("order: the column passes over the rows do not give the order of sort_records_host_by_name");
    size_t at = 0;
    for (size_t k = 0; k < N; ++k) { if (std::memcmp(dst.data() + at, bytes.data() + sorted[k].off, sorted[k].len) != 0) return fail("order: the gathered bytes"); at += sorted[k].len; }
    std::printf("order ok: %zu records, rows of %u words\n", N, W);
    size_t x = 0;
    while (x + 1 < N && bam_name_cmp(names[by_rows[x]].c_str(), names[by_rows[x + 1]].c_str()) == 0) ++x;
    std::swap(by_rows[x], by_rows[x + 1]);
    if (same(by_rows)) return fail("swap: a swapped pair went unnoticed");
    std::printf("swap ok: one swapped pair fails the comparison\n");
    return 0;
}

int main()
{
    if (check_exhaustive() || check_random() || check_length() || check_order()) return 1;
    std::printf("all ok\n");
    return 0;
}
