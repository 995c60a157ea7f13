// bamsink_check.cpp -- every writer of csrc/ps_bam.cpp driven on the host, through ps_bam.h's public interface alone, into a directory
// given on the command line.  tests/test_bam_writer_stable_cpu.py holds what the files inflate to against tests/golden/
// bam_writer_streams.json; this program checks what needs the library itself: that a kept BamFile is the file's records in file order.
// Built with AddressSanitizer and UBSan as a plain executable, with ps_bam.cpp and zlib.
//
// The records: 3,000 of them, seeded.  All but a few take 120 bytes, and 0xff00 is 544 times 120: in any order the first blocks end
// exactly where a record ends and the next record starts exactly on the cut.  A few records are 7 bytes longer; they lie behind the
// first cut in input order, in coordinate order (reference 1) and in name order (numbers in the middle of the range), so that every
// record behind them that meets a cut straddles it.  shape() checks that for the input and for both kept files.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "ps_bam.h"
#include "ps_error.h"

using namespace ps;

static int fail(const std::string &m) { std::printf("FAIL %s\n", m.c_str()); return 1; }

struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } };

static const size_t BLK = 0xff00, N = 3000, LEN = 120;
typedef std::vector<std::pair<std::string, uint32_t>> Refs;
static const Refs kRefs = {{"c0", 400000}, {"c1", 900000}, {"c2", 200000}};

struct Made { std::string bytes; std::vector<BamRec> recs; std::string sam; };

// record i: name r<number>, one CIGAR word, 36 bases, NM:i and an XZ:Z tag that pads the record to LEN (LEN + 7 for the long ones)
static void make_record(Rng &g, size_t i, Made &m, std::string *prev_name)
{
    const bool longer = i >= 700 && i % 500 == 3;
    const bool second = prev_name && i % 10 == 9 && !longer;                 // the second read of a pair: the name of the record before
    char name[32];
    if (second) std::snprintf(name, sizeof name, "%s", prev_name->c_str());
    else std::snprintf(name, sizeof name, "r%u", longer ? 5000000u + (unsigned)i : g.next() % (i % 3 == 0 ? 1000u : 10000000u));
    const bool placed = g.next() % 20 != 0;
    BamCore c{};
    c.ref = !placed ? -1 : longer ? 1 : (int32_t)(g.next() % 3); c.pos = placed ? (int32_t)(g.next() % (kRefs[(size_t)c.ref].second - 40)) : -1;
    c.end = (int64_t)c.pos + (placed ? 36 : 1); c.mapq = placed ? (int)(g.next() % 61) : 0;
    c.flag = (placed ? (int)(g.next() % 2) * 16 : 4) | (second ? 0x81 : i % 10 == 8 ? 0x41 : 0);
    c.n_cigar = placed ? 1 : 0; c.l_seq = 36;
    BamRec r;
    bam_rec_begin(m.bytes, c, name, std::strlen(name), r);
    const uint32_t word = 36u << 4;
    if (placed) bam_rec_cigar(m.bytes, &word, 1);
    std::string seq, qual;
    for (int j = 0; j < 36; ++j) { seq.push_back("ACGT"[g.next() % 4]); qual.push_back((char)(33 + g.next() % 41)); }
    for (int j = 0; j < 36; j += 2) m.bytes.push_back((char)(uint8_t)(((1 << (std::strchr("ACGT", seq[j]) - "ACGT")) << 4) | (1 << (std::strchr("ACGT", seq[j + 1]) - "ACGT"))));
    for (int j = 0; j < 36; ++j) m.bytes.push_back((char)(qual[j] - 33));
    const int nm = (int)(g.next() % 200);
    bam_tag_int(m.bytes, "NM", nm);
    const size_t have = m.bytes.size() - r.off, want = LEN + (longer ? 7 : 0);
    std::string pad(want - have - 4, 'x');
    for (char &ch : pad) ch = (char)('a' + g.next() % 26);
    bam_tag_text(m.bytes, "XZ", 'Z', pad.data(), pad.size());
    bam_rec_end(m.bytes, r);
    r.part = 0;
    m.recs.push_back(r);
    m.sam += std::string(name) + "\t" + std::to_string(c.flag) + "\t" + (placed ? kRefs[(size_t)c.ref].first : "*") + "\t" + std::to_string(c.pos + 1) + "\t" + std::to_string(c.mapq) + "\t" +
             (placed ? "36M" : "*") + "\t*\t0\t0\t" + seq + "\t" + qual + "\tNM:i:" + std::to_string(nm) + "\tXZ:Z:" + pad + "\n";
    if (prev_name) *prev_name = name;
}

static Made make_records(size_t n, uint64_t seed)
{
    Made m; Rng g{seed}; std::string prev;
    for (size_t i = 0; i < n; ++i) make_record(g, i, m, &prev);
    return m;
}

// of records back to back in this order: three or more blocks, a record that ends exactly on a cut, one that starts on one, some that straddle one
static bool shape(const std::vector<BamRec> &recs, const char *what)
{
    uint64_t at = 0; size_t ends = 0, starts = 0, straddles = 0;
    for (const BamRec &r : recs) {
        const uint64_t e = at + r.len;
        if (at && at % BLK == 0) ++starts;
        if (e % BLK == 0) ++ends;
        if (at / BLK != (e - 1) / BLK) ++straddles;
        at = e;
    }
    if (at <= 2 * BLK || !ends || !starts || straddles < 2) { std::printf("FAIL shape of %s: %llu bytes, %zu end on a cut, %zu start on one, %zu straddle one\n", what, (unsigned long long)at, ends, starts, straddles); return false; }
    return true;
}

static std::string header_text(const Refs &refs, size_t comment_bytes)
{
    std::string t = "@HD\tVN:1.6\tSO:unsorted\n";
    for (auto &r : refs) t += "@SQ\tSN:" + r.first + "\tLN:" + std::to_string(r.second) + "\n";
    for (size_t k = 0; t.size() < comment_bytes; ++k) t += "@CO\tline " + std::to_string(k) + " of a header that takes more than one block\n";
    return t;
}

// the records of [i0, i1) as a buffer of their own, offsets from its start
static void slice(const Made &m, size_t i0, size_t i1, std::string &bytes, std::vector<BamRec> &recs)
{
    const size_t b0 = i0 < m.recs.size() ? m.recs[i0].off : m.bytes.size(), b1 = i1 < m.recs.size() ? m.recs[i1].off : m.bytes.size();
    bytes.assign(m.bytes, b0, b1 - b0);
    recs.assign(m.recs.begin() + (long)i0, m.recs.begin() + (long)i1);
    for (BamRec &r : recs) r.off -= b0;
}

// the kept records are the file's records, in file order, and every one lies where its BamRec says
static bool kept_is_the_file(const BamFile &kept, const std::string &path, const char *order)
{
    BamFile f;
    load_records(path.c_str(), 2, f);
    if (kept.sort_order != order || f.sort_order != order || kept.text != f.text || kept.refs != f.refs || kept.n() != f.n()) { std::printf("FAIL kept %s: header or count\n", path.c_str()); return false; }
    for (size_t i = 0; i < f.n(); ++i) {
        const BamRec &a = kept.recs[i], &b = f.recs[i];
        if (a.part < 0 || (size_t)a.part >= kept.enc.size() || a.off + a.len > kept.enc[(size_t)a.part].size()) { std::printf("FAIL kept %s: record %zu lies outside its part\n", path.c_str(), i); return false; }
        if (a.len != b.len || a.ref != b.ref || a.pos != b.pos || a.end != b.end || a.flag != b.flag || std::memcmp(kept.rec(i), f.rec(i), a.len) != 0) { std::printf("FAIL kept %s: record %zu\n", path.c_str(), i); return false; }
    }
    return shape(kept.recs, path.c_str());
}

static void write_file(const std::string &path, const std::string &text)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(text.data(), 1, text.size(), f) != text.size() || std::fclose(f) != 0) throw Error("cannot write " + path);
}

static int run(const std::string &dir)
{
    const Made m = make_records(N, 20261021);
    if (!shape(m.recs, "the input")) return 1;
    const std::string text = header_text(kRefs, 0);
    auto at = [&](const char *name) { return dir + "/" + name; };
    BamStats st;

    // ---- unsorted, the span overload: two buffers, cut where a record ends
    {
        BamSink sink(text, kRefs, at("unsorted_span.bam").c_str(), false, false, 3, 6);
        for (size_t i0 = 0; i0 < N; i0 += 1700) {
            std::string bytes; std::vector<BamRec> recs;
            slice(m, i0, std::min(N, i0 + 1700), bytes, recs);
            sink.add(bytes.data(), bytes.size(), recs, recs.size() + 1);
        }
        sink.finish(&st);
        if (st.n_out != N || st.n_in != N + 2) return fail("unsorted_span: counts");
    }
    // ---- unsorted, the vector overload: two calls, four buffers (one empty) and two
    {
        BamSink sink(text, kRefs, at("unsorted_vec.bam").c_str(), false, false, 3, 6);
        const size_t cut[] = {0, 600, 600, 1300, 1301, 2400, N};
        for (size_t c0 : {(size_t)0, (size_t)4}) {
            const size_t c1 = c0 == 0 ? 4 : 6;
            std::vector<std::string> bytes(c1 - c0); std::vector<std::vector<BamRec>> recs(c1 - c0);
            for (size_t k = c0; k < c1; ++k) slice(m, cut[k], cut[k + 1], bytes[k - c0], recs[k - c0]);
            sink.add(bytes, recs, cut[c1] - cut[c0]);
            if (!bytes.empty() || !recs.empty()) return fail("unsorted_vec: add() did not consume its buffers");
        }
        sink.finish(&st);
        if (st.n_out != N || st.n_in != N) return fail("unsorted_vec: counts");
    }
    // ---- sorted: by coordinate with index, by name; each once more with the records kept
    for (int mode = 0; mode < 4; ++mode) {
        const bool by_name = mode & 1, keep = mode & 2;
        const std::string path = at(by_name ? (keep ? "name_keep.bam" : "name.bam") : (keep ? "coord_keep.bam" : "coord.bam"));
        BamSink sink(text, kRefs, path.c_str(), !by_name, !by_name, 3, 6, by_name);
        std::vector<std::string> bytes(2); std::vector<std::vector<BamRec>> recs(2);
        slice(m, 0, 1100, bytes[0], recs[0]); slice(m, 1100, 1100, bytes[1], recs[1]);
        sink.add(bytes, recs, 1100);
        std::string more; std::vector<BamRec> more_recs;
        slice(m, 1100, N, more, more_recs);
        sink.add(more.data(), more.size(), more_recs, N - 1100);
        BamFile kept;
        sink.finish(&st, keep ? &kept : nullptr);
        if (st.n_out != N || st.n_in != N) return fail(path + ": counts");
        if (keep && !kept_is_the_file(kept, path, by_name ? "queryname" : "coordinate")) return 1;
    }
    // ---- empty sinks
    { BamSink sink(text, kRefs, at("empty.bam").c_str(), false, false, 3, 6); sink.finish(&st); if (st.n_out || st.n_in) return fail("empty: counts"); }
    { BamSink sink(text, kRefs, at("empty_coord.bam").c_str(), true, true, 3, 6); BamFile kept; sink.finish(&st, &kept); if (st.n_out || kept.n()) return fail("empty_coord: counts"); }
    // ---- a header of two blocks, through the sink's own header path and through the sorted writer's
    {
        const std::string big = header_text(kRefs, BLK + 5000);
        const Made few = make_records(40, 7);
        for (int sorted = 0; sorted < 2; ++sorted) {
            BamSink sink(big, kRefs, at(sorted ? "bighead_coord.bam" : "bighead.bam").c_str(), sorted != 0, sorted != 0, 2, 6);
            std::string bytes; std::vector<BamRec> recs;
            slice(few, 0, 40, bytes, recs);
            sink.add(bytes.data(), bytes.size(), recs, 40);
            sink.finish(&st);
            if (st.n_out != 40) return fail("bighead: counts");
        }
    }
    // ---- the file-to-file writers, on a SAM of the same records
    {
        const Made s = make_records(1800, 99);
        write_file(at("in.sam"), text + s.sam);
        sam_to_bam(at("in.sam").c_str(), at("s2b.bam").c_str(), 0, false, false, 3, &st);
        if (st.n_in != 1800 || st.n_out != 1800) return fail("sam_to_bam: counts");
        sam_to_bam(at("in.sam").c_str(), at("s2b_sorted.bam").c_str(), 0, true, true, 3, &st);
        sam_to_bam(at("in.sam").c_str(), at("s2b_q20.bam").c_str(), 20, false, false, 2, &st);
        if (st.n_in != 1800 || st.n_out == 0 || st.n_out >= 1800) return fail("sam_to_bam -q: counts");
        bam_view(at("s2b.bam").c_str(), at("view_q30.bam").c_str(), 30, 3, &st);
        if (st.n_out == 0 || st.n_out >= 1800) return fail("bam_view: counts");
        bam_sort(at("s2b.bam").c_str(), at("sort_coord.bam").c_str(), false, 3, &st);
        bam_sort(at("s2b.bam").c_str(), at("sort_name.bam").c_str(), true, 3, &st);
        bam_sort(at("s2b.bam").c_str(), at("indexed.bam").c_str(), false, 1, &st);
        bam_index(at("indexed.bam").c_str(), 3);
        ExtractStats es;
        extract_weak_reads(at("s2b.bam").c_str(), at("weak_rest.bam").c_str(), at("weak.fq").c_str(), 25, 3, &es);
        if (es.n_records != 1800 || es.n_weak == 0 || es.n_weak + es.n_kept != 1800) return fail("extract_weak_reads: counts");
    }
    std::printf("all ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return fail("usage: bamsink_check <directory>");
    try { return run(argv[1]); } catch (const std::exception &e) { return fail(e.what()); }
}
