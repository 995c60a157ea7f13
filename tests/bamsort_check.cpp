// bamsort_check.cpp -- csrc/ps_bamsort.h under the host compiler alone (tests/test_bamsort_cpu.py builds it with AddressSanitizer
// and UBSan, together with csrc/ps_bam.cpp, and runs it as a plain program).
//   keys    the permutation of a plain std::stable_sort on ps_bamsort.h's 64-bit keys against the one ps_bam.cpp's host route makes
//           (sort_records_host: the comparator of sort_records), on 20,000 seeded records; the same with the keys cut at
//           bamsort_end_bit, as the device sort is bounded.
//   gather  the group of 64 lanes run lane by lane over every group of a seeded set of records, on heap buffers of the exact
//           size (the source up to a multiple of 4, as the header asks), over two backgrounds: after every group the bytes of its
//           range are the reference's and every other byte still has the value it had before the group.
//   swap    negative control: one swapped pair in the permutation must fail the comparison.
//   piece   PS_BAM_SORT_PIECE's parser at every documented clamp; the four column sub-arrays of a half (no overlap, inside the half,
//           aligned) for every piece size from 256 to 8192 and the default; a replay of run_route's upload loop over ps_bamsort.h's
//           cut: the copies tile the parts' bytes once and in order, for part lists with empty parts, parts that end on a piece
//           boundary and parts of many pieces.
#include <algorithm>
#include <utility>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ps_bam.h"
#include "ps_bamsort.h"

using namespace ps;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }
static int fail(const char *what) { std::fprintf(stderr, "FAIL %s\n", what); return 1; }

// ------------------------------------------------------------------ keys
static int check_keys()
{
    const size_t N = 20000;
    std::vector<BamRec> recs(N);
    size_t i = 0;
    auto put = [&](int32_t ref, int32_t pos) { BamRec r; r.ref = ref; r.pos = pos; r.end = pos; r.flag = 0; r.off = i; r.len = 0; r.part = 0; recs[i++] = r; };
    const int32_t edge_pos[] = {0, 0x7fffffff, 1, 0x7ffffffe, 12345};
    const int32_t edge_ref[] = {0, 70000, 1, 69999};
    for (int32_t ref : edge_ref) for (int32_t pos : edge_pos) put(ref, pos);
    for (int run = 0; run < 4; ++run) {                                         // runs of 500 equal keys, one of them unplaced, not adjacent in the input
        const int32_t ref = run == 3 ? -1 : (int32_t)below(70001), pos = run == 3 ? -1 : (int32_t)below(0x7fffffff);
        for (int k = 0; k < 500; ++k) put(ref, pos);
    }
    while (i < N) {
        const uint32_t kind = below(10);
        if (kind == 0) put(-1, -1);                                             // unplaced, scattered among the placed
        else if (kind == 1) put((int32_t)below(70001), below(2) ? 0 : 0x7fffffff);
        else if (kind == 2) put(below(2) ? 0 : 70000, (int32_t)below(0x7fffffff));
        else put((int32_t)below(8), (int32_t)below(3000));                      // many ties
    }
    for (size_t k = N - 1; k > 0; --k) std::swap(recs[k], recs[below((uint32_t)k + 1)]);
    for (size_t k = 0; k < N; ++k) recs[k].off = k;                            // off: the record's place in the input
    std::vector<uint64_t> key(N); uint64_t any = 0;
    for (size_t k = 0; k < N; ++k) { key[k] = bamsort_key(recs[k].ref, recs[k].pos); any |= key[k]; }
    std::vector<uint32_t> by_key(N), by_cut(N);
    for (size_t k = 0; k < N; ++k) by_key[k] = by_cut[k] = (uint32_t)k;
    std::stable_sort(by_key.begin(), by_key.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
    const int end_bit = bamsort_end_bit(any);
    if (end_bit != 64) return fail("keys: with unplaced records every bit of the key counts");
    if (bamsort_end_bit(bamsort_key(5, 0x7fffffff)) != 35 || bamsort_end_bit(bamsort_key(0, 0)) != 32 || bamsort_end_bit(0) != 1) return fail("keys: end bit");
    const uint64_t mask = end_bit >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << end_bit) - 1);
    std::stable_sort(by_cut.begin(), by_cut.end(), [&](uint32_t x, uint32_t y) { return (key[x] & mask) < (key[y] & mask); });
    std::vector<char> bytes(N + 1, 0); char none = 0;
    sort_records_host(bytes.data(), recs, 3, &none);                            // the library's comparator; the records have no bytes
    size_t unplaced_first = N;
    for (size_t k = 0; k < N; ++k) {
        if (recs[k].off != by_key[k] || by_cut[k] != by_key[k]) return fail("keys: the order of the keys is not the order of sort_records");
        if (recs[k].ref == -1 && unplaced_first == N) unplaced_first = k;
        if (unplaced_first != N && recs[k].ref != -1) return fail("keys: an unplaced record before a placed one");
    }
    if (unplaced_first == N || recs[0].ref != 0 || recs[0].pos != 0) return fail("keys: the edge records are not where they belong");
    std::printf("keys ok: %zu records, %zu unplaced at the end, end bit %d\n", N, N - unplaced_first, end_bit);
    return 0;
}

// ------------------------------------------------------------------ gather
struct Case { std::vector<uint64_t> off; std::vector<uint32_t> len, perm; std::vector<uint64_t> doff; uint8_t *src = nullptr, *ref = nullptr; size_t src_bytes = 0, out_bytes = 0; uint64_t d0 = 0; };

static void *exact(size_t bytes) { void *p = nullptr; if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) std::abort(); return p; }

// lens in input order; every record lies behind a gap of 0 to 3 bytes; the destination starts at d0
static void make_case(Case &c, const std::vector<uint32_t> &lens, uint64_t d0)
{
    const size_t n = lens.size();
    c.len = lens; c.off.resize(n); c.perm.resize(n); c.doff.resize(n + 1); c.d0 = d0;
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) { at += below(4); c.off[i] = at; at += lens[i]; }
    c.src_bytes = (size_t)((at + 3) & ~(uint64_t)3);
    c.src = (uint8_t *)exact(c.src_bytes);
    for (size_t b = 0; b < c.src_bytes; ++b) c.src[b] = (uint8_t)rnd();
    for (size_t i = 0; i < n; ++i) c.perm[i] = (uint32_t)i;
    for (size_t k = n; k > 1; --k) std::swap(c.perm[k - 1], c.perm[below((uint32_t)k)]);
    c.doff[0] = d0;
    for (size_t i = 0; i < n; ++i) c.doff[i + 1] = c.doff[i] + lens[c.perm[i]];
    c.out_bytes = (size_t)c.doff[n];
    c.ref = (uint8_t *)exact(c.out_bytes);
    for (size_t i = 0; i < n; ++i) std::memcpy(c.ref + c.doff[i], c.src + c.off[c.perm[i]], lens[c.perm[i]]);
}
static void free_case(Case &c) { std::free(c.src); std::free(c.ref); c.src = c.ref = nullptr; }

// every group over both backgrounds; perm: the permutation handed to the gather (the reference was made with c.perm)
static bool gather_equals_reference(const Case &c, const std::vector<uint32_t> &perm, bool verbose)
{
    const size_t n = c.len.size();
    BsShared *sh = (BsShared *)exact(sizeof(BsShared));
    uint8_t *out = (uint8_t *)exact(c.out_bytes), *before = (uint8_t *)exact(c.out_bytes);
    bool ok = true;
    for (int bg = 0; bg < 2 && ok; ++bg) {
        std::memset(out, bg ? 0x5a : 0xa5, c.out_bytes);
        BsArgs a{c.src, c.off.data(), c.len.data(), perm.data(), c.doff.data(), (uint64_t)n, out};
        for (uint64_t g0 = 0; g0 < n && ok; g0 += BS_NL) {
            std::memcpy(before, out, c.out_bytes);
            std::memset(sh, 0xcc, sizeof(BsShared));
            bamsort_gather_group(*sh, a, g0);
            const uint64_t beg = c.doff[g0], end = c.doff[std::min<uint64_t>(n, g0 + BS_NL)];
            for (uint64_t b = 0; b < c.out_bytes; ++b) {
                const uint8_t want = b >= beg && b < end ? c.ref[b] : before[b];
                if (out[b] != want) { if (verbose) std::fprintf(stderr, "group at %llu, background %d: byte %llu is %02x, not %02x (range %llu..%llu)\n", (unsigned long long)g0, bg, (unsigned long long)b, out[b], want, (unsigned long long)beg, (unsigned long long)end); ok = false; break; }
            }
        }
        if (ok && std::memcmp(out + c.d0, c.ref + c.d0, c.out_bytes - c.d0) != 0) ok = false;
    }
    std::free(out); std::free(before); std::free(sh);
    return ok;
}

static int check_gather()
{
    bool seen[16][16]; std::memset(seen, 0, sizeof seen);
    size_t n_cases = 0, n_records = 0;
    for (uint64_t d0 = 0; d0 < 16; ++d0) {
        std::vector<uint32_t> lens;
        for (uint32_t l = 36; l <= 900; ++l) lens.push_back(l);                 // every length once ...
        for (int k = 0; k < 200; ++k) lens.push_back(36 + below(200));          // ... and the common ones again
        for (size_t k = lens.size(); k > 1; --k) std::swap(lens[k - 1], lens[below((uint32_t)k)]);
        if (d0 % 4 != 3) lens.insert(lens.begin() + (d0 % 4 == 0 ? 0 : d0 % 4 == 1 ? lens.size() / 2 : lens.size()), 70000u);   // the one large record: first, middle, last, none
        Case c; make_case(c, lens, d0);
        for (size_t i = 0; i < lens.size(); ++i) seen[c.off[c.perm[i]] & 15][c.doff[i] & 15] = true;
        const bool ok = gather_equals_reference(c, c.perm, true);
        ++n_cases; n_records += lens.size();
        free_case(c);
        if (!ok) return fail("gather: a byte differs from the reference or was written outside the group's range");
    }
    for (int s = 0; s < 16; ++s) for (int d = 0; d < 16; ++d) if (!seen[s][d]) return fail("gather: a pair of residues mod 16 was not covered");
    // the sizes around one group, and groups of records that alone fill the staging
    const size_t small[] = {1, 2, 63, 64, 65, 129};
    for (size_t n : small) {
        std::vector<uint32_t> lens(n);
        for (auto &l : lens) l = 36 + below(300);
        Case c; make_case(c, lens, below(16));
        const bool ok = gather_equals_reference(c, c.perm, true);
        free_case(c); ++n_cases; n_records += n;
        if (!ok) return fail("gather: a small case");
    }
    {
        std::vector<uint32_t> lens = {BS_STAGE, BS_STAGE - 15, BS_STAGE + 1, 36, BS_STAGE - 16, 40, 41, BS_STAGE / 2, BS_STAGE / 2 + 7, 37};
        for (uint64_t d0 = 0; d0 < 16; d0 += 5) {
            Case c; make_case(c, lens, d0);
            const bool ok = gather_equals_reference(c, c.perm, true);
            free_case(c); ++n_cases; n_records += lens.size();
            if (!ok) return fail("gather: records of about the staging's size");
        }
    }
    std::printf("gather ok: %zu cases, %zu records, all 256 pairs of source and destination residues mod 16\n", n_cases, n_records);
    return 0;
}

static int check_swap()
{
    std::vector<uint32_t> lens(200);
    for (auto &l : lens) l = 36 + below(100);
    lens[10] = lens[11] = 77;                                                   // same length: the offsets stay, only the bytes move
    Case c; make_case(c, lens, 3);
    std::vector<uint32_t> perm = c.perm;
    size_t x = 0, y = 0;
    for (size_t i = 0; i < perm.size(); ++i) { if (perm[i] == 10) x = i; if (perm[i] == 11) y = i; }
    const bool good = gather_equals_reference(c, perm, true);
    std::swap(perm[x], perm[y]);
    const bool bad = gather_equals_reference(c, perm, false);
    free_case(c);
    if (!good) return fail("swap: the unswapped permutation");
    if (bad) return fail("swap: a swapped pair went unnoticed");
    std::printf("swap ok: one swapped pair fails the comparison\n");
    return 0;
}

// ------------------------------------------------------------------ the staging: knob, column layout, upload cut
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// the piece size with PS_BAM_SORT_PIECE set to `value` (nullptr: unset), read from the environment as run_route reads it
static size_t with(const char *value)
{
    unsetenv("PS_BAM_SORT_PIECE");
    if (value) setenv("PS_BAM_SORT_PIECE", value, 1);
    return bamsort_piece_bytes(std::getenv("PS_BAM_SORT_PIECE"));
}

static int check_piece_knob()
{
    const size_t D = (size_t)64 << 20;
    CHECK(BS_PIECE_DEFAULT == D && D % 64 == 0);
    CHECK(with(nullptr) == D); CHECK(with("") == D); CHECK(with("abc") == D); CHECK(with("0") == D); CHECK(with("-5") == D);     // the default
    CHECK(with("1") == 256); CHECK(with("255") == 256); CHECK(with("256") == 256);                                             // at least 256
    CHECK(with("257") == 256); CHECK(with("319") == 256); CHECK(with("320") == 320);                                           // down to a multiple of 64
    CHECK(with("67108864") == D); CHECK(with("67108865") == D); CHECK(with("99999999999") == D);                               // never more than the default
    CHECK(with("4096") == 4096); CHECK(with("67108863") == D - 64);
    unsetenv("PS_BAM_SORT_PIECE");
    std::printf("piece knob ok: 16 values\n");
    return 0;
}

static int check_one_layout(size_t piece)
{
    const size_t per = bamsort_columns_per_piece(piece);
    const BsColumnsAt c = bamsort_columns_at(per);
    CHECK(per >= 1);
    const size_t beg[4] = {c.off, c.len, c.ref, c.pos}, width[4] = {8, 4, 4, 4};
    for (int a = 0; a < 4; ++a) {
        CHECK(beg[a] + width[a] * per <= piece);                                  // ends inside the half
        CHECK(beg[a] % width[a] == 0);                                            // a half starts at a multiple of 64: the offset's alignment is the array's
        for (int b = 0; b < a; ++b) CHECK(beg[b] + width[b] * per <= beg[a] || beg[a] + width[a] * per <= beg[b]);
    }
    return 0;
}

static int check_column_layout()
{
    size_t n = 0;
    for (size_t piece = 256; piece <= 8192; piece += 64, ++n) if (check_one_layout(piece)) return 1;
    if (check_one_layout(BS_PIECE_DEFAULT)) return 1;
    CHECK(bamsort_columns_per_piece(256) == 12 && bamsort_columns_per_piece(BS_PIECE_DEFAULT) == 3355443);
    CHECK(BS_PIECE_DEFAULT % 64 == 0);                                            // the second half starts aligned as the first
    std::printf("column layout ok: %zu piece sizes and the default\n", n);
    return 0;
}

// The upload loop of run_route with its copies recorded in place of made: per piece the (device offset, bytes) of the one copy to the
// device, and per cut the source range it takes.  The cut itself is ps_bamsort.h's.
struct Replay { std::vector<std::pair<uint64_t, size_t>> copies; bool ok = true; size_t n_cuts = 0; };
static Replay replay_upload(const std::vector<uint64_t> &parts, size_t piece)
{
    Replay r;
    uint64_t src_bytes = 0;
    std::vector<uint64_t> base;
    for (uint64_t n : parts) { base.push_back(src_bytes); src_bytes += n; }
    BsCursor cur; uint64_t at = 0;
    while (at < src_bytes) {
        size_t fill = 0;
        while (fill < piece && cur.part < parts.size()) {
            const BsCut c = bamsort_next_cut(cur, parts[cur.part], piece - fill);
            ++r.n_cuts;
            // the cut lies inside its part, fits the half, and is the next source byte in the back-to-back order
            if (c.part >= parts.size() || c.in_part + c.take > parts[c.part] || c.take > piece - fill || base[c.part] + c.in_part != at + fill) r.ok = false;
            if (c.take == 0 && parts[c.part] != 0) r.ok = false;                  // only an empty part yields nothing
            fill += c.take;
        }
        if (fill == 0) { r.ok = false; break; }
        r.copies.push_back({at, fill});
        at += fill;
    }
    if (cur.in_part != 0) r.ok = false;
    for (size_t k = cur.part; k < parts.size(); ++k) if (parts[k] != 0) r.ok = false;      // only empty parts may be left behind the last byte
    return r;
}

static int check_upload_cut()
{
    const size_t pieces[] = {256, 320, 4096};
    size_t n_cases = 0;
    for (size_t P : pieces) {
        const std::vector<std::vector<uint64_t>> lists = {
            {},                                                                   // nothing at all
            {0}, {0, 0, 0},                                                       // only empty parts
            {1}, {P - 1}, {P}, {P + 1},                                           // around one piece
            {P, P}, {2 * P}, {P / 2, P / 2, P},                                   // parts that end exactly on a piece boundary
            {0, 5, 0, 0, P, 0, 7, 0},                                             // empty parts first, between and last
            {37 * P + 11},                                                        // one part of many pieces
            {3, 10 * P + 1, 0, P - 4, 1, 1, 1, 5 * P},                            // pieces that span several parts, parts that span several pieces
        };
        for (const auto &parts : lists) {
            uint64_t src_bytes = 0;
            for (uint64_t n : parts) src_bytes += n;
            const Replay r = replay_upload(parts, P);
            CHECK(r.ok);
            CHECK(r.copies.size() == (src_bytes + P - 1) / P);
            uint64_t at = 0;
            for (size_t k = 0; k < r.copies.size(); ++k) {                        // the copies tile [0, src_bytes) once and in order, every piece but the last full
                CHECK(r.copies[k].first == at && r.copies[k].second >= 1 && r.copies[k].second <= P);
                CHECK(k + 1 == r.copies.size() || r.copies[k].second == P);
                at += r.copies[k].second;
            }
            CHECK(at == src_bytes);
            ++n_cases;
        }
    }
    {   // seeded lists, a third of the parts empty
        for (int t = 0; t < 200; ++t) {
            const size_t P = 256 + 64 * below(8);
            std::vector<uint64_t> parts(1 + below(9));
            uint64_t src_bytes = 0;
            for (auto &n : parts) { n = below(3) == 0 ? 0 : below(2) ? below(4 * (uint32_t)P) : (uint64_t)P * below(4); src_bytes += n; }
            const Replay r = replay_upload(parts, P);
            CHECK(r.ok && r.copies.size() == (src_bytes + P - 1) / P);
            uint64_t at = 0;
            for (const auto &c : r.copies) { CHECK(c.first == at && c.second >= 1 && c.second <= P); at += c.second; }
            CHECK(at == src_bytes);
            ++n_cases;
        }
    }
    std::printf("upload cut ok: %zu part lists\n", n_cases);
    return 0;
}

int main()
{
    if (check_keys() || check_gather() || check_swap()) return 1;
    if (check_piece_knob() || check_column_layout() || check_upload_cut()) return 1;
    std::printf("all ok\n");
    return 0;
}
