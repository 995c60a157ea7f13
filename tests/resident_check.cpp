// resident_check.cpp -- drives csrc/ps_resident.h alone (tests/test_resident_cpu.py): keys, the identity of the index files, the
// LRU bound, drop-after-error, the end of a scope and who holds a device's lanes of work, with stub payloads and stub closers.
// A plain program: every check that fails prints what it expected and ends the run with status 1.
#include <cstdio>
#include <fstream>
#include <set>
#include <unistd.h>
#include "ps_resident.h"

using namespace ps;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Stub { int id = -1; std::vector<int> devs; std::set<int> lanes; };      // lanes: the devices whose lanes of work this payload holds
typedef ResidentCache<Stub> Cache;

struct Bench {
    Cache c; int next_id = 0; std::map<int, int> closed; int closes_seen = 0;
    Bench()
    {
        c.close = [this](Stub &gone, Stub *heir) {
            ++closed[gone.id]; ++closes_seen;
            if (heir) for (int d : heir->devs) if (gone.lanes.count(d)) { gone.lanes.erase(d); heir->lanes.insert(d); }
            gone.lanes.clear();                    // what no heir took is freed
        };
    }
    // never two holders of a device's lanes, and the holder is the one the books name
    void lanes_ok()
    {
        std::map<int, int> holders;
        for (auto &e : c.entries) for (int d : e->payload.lanes) {
            CHECK(++holders[d] == 1);
            CHECK(c.lane_owner.count(d) && c.lane_owner[d] == e.get());
        }
        for (auto &o : c.lane_owner) { bool live = false; for (auto &e : c.entries) live = live || e.get() == o.second; CHECK(live); }
    }
    // what a mapping call does with an entry before its pass: look up, take the lanes over, make those that are missing
    Cache::Entry *use(const ResidentKey &k, const ResidentIdent &id)
    {
        Cache::Entry *e = c.acquire(k, id, [&](Stub &s) { s.id = next_id++; s.devs = k.devs; });
        lanes_ok();
        for (Cache::Entry *f : c.take_lanes(e)) {
            CHECK(f != e);
            for (int d : e->payload.devs) if (f->payload.lanes.count(d)) { f->payload.lanes.erase(d); e->payload.lanes.insert(d); }
        }
        for (int d : e->payload.devs) e->payload.lanes.insert(d);
        lanes_ok();
        return e;
    }
    int call(const ResidentKey &k, const ResidentIdent &id, bool ok = true)
    {
        Cache::Entry *e = use(k, id);
        const int pid = e->payload.id;
        if (ok) c.release(e); else c.drop(e);
        lanes_ok();
        return pid;
    }
    int n_closed() const { int n = 0; for (auto &x : closed) { CHECK(x.second == 1); n += x.second; } return n; }   // nothing is closed twice
};

static ResidentKey key(const std::string &path, const char *ids, const ResidentKnobs &kn = ResidentKnobs())
{
    return resident_key(path.c_str(), plan_devices(ids, 1, 1, 8, 4), kn);
}
static ResidentIdent ident(int seed)
{
    ResidentIdent id;
    for (int f = 0; f < 4; ++f) { FileIdent x; x.dev = 7; x.ino = (uint64_t)(100 * seed + f); x.size = 1000 + f; x.mtime_s = 5000; x.mtime_ns = 123456789; id.files.push_back(x); }
    return id;
}
static void write_file(const std::string &p, const std::string &text) { std::ofstream f(p, std::ios::binary); f << text; CHECK(f.good()); }

static void keys(const std::string &dir)
{
    const std::string fa = dir + "/ref.fa";
    write_file(fa, ">a\nACGT\n");
    CHECK(::symlink("ref.fa", (dir + "/link.fa").c_str()) == 0);
    CHECK(::mkdir((dir + "/sub").c_str(), 0755) == 0);
    // the path spelled several ways is one key; another file is another
    CHECK(key(fa, "0") == key(dir + "/./ref.fa", "0"));
    CHECK(key(fa, "0") == key(dir + "/sub/../ref.fa", "0"));
    CHECK(key(fa, "0") == key(dir + "/link.fa", "0"));
    write_file(dir + "/other.fa", ">a\nACGT\n");
    CHECK(!(key(fa, "0") == key(dir + "/other.fa", "0")));
    // index files without a FASTA: by the .ann file; nothing at all: as spelled
    write_file(dir + "/only.ann", "x");
    CHECK(resident_path((dir + "/./only").c_str()) == resident_path((dir + "/only").c_str()) && resident_path((dir + "/./only").c_str()).find("/./") == std::string::npos);
    CHECK(resident_path("no/such/./file") == "no/such/./file");
    // the device plan: one worker on device 0 is not two workers on device 0, nor device 1; not stated is device 0
    CHECK(!(key(fa, "0") == key(fa, "0,0")));
    CHECK(!(key(fa, "0") == key(fa, "1")));
    CHECK(!(key(fa, "0,1") == key(fa, "1,0")));
    CHECK(key(fa, "0") == key(fa, nullptr));
    CHECK(key(fa, "0,0") == resident_key(fa.c_str(), plan_devices("0", 1, 2, 8, 4), ResidentKnobs()));     // PS_WORKERS_PER_GPU=2: the same plan
    // each knob
    ResidentKnobs base;
    for (int f = 0; f < 5; ++f) {
        ResidentKnobs k = base;
        (f == 0 ? k.jump : f == 1 ? k.jump_levels : f == 2 ? k.pool_cap : f == 3 ? k.n_big : k.bt_blocks) += 1;
        CHECK(!(key(fa, "0", k) == key(fa, "0", base)));
        CHECK(resident_fingerprint(k) != resident_fingerprint(base));
    }
    ResidentKnobs a, b; a.jump_levels = 5; b.jump_levels = 6;
    CHECK(!(key(fa, "0", a) == key(fa, "0", b)) && key(fa, "0", a) == key(fa, "0", a));
    a = base; b = base; a.pool_cap = 1; a.n_big = 0; b.pool_cap = 0; b.n_big = 1;        // not a sum of the values
    CHECK(resident_fingerprint(a) != resident_fingerprint(b));
    // under unequal keys a scope holds two entries, under equal ones one
    Bench t; std::string err;
    CHECK(t.c.begin(8, err));
    const int p0 = t.call(key(fa, "0"), ident(1));
    CHECK(t.call(key(dir + "/link.fa", "0"), ident(1)) == p0);
    CHECK(t.call(key(fa, "0,0"), ident(1)) != p0);
    CHECK(t.call(key(fa, "0", a), ident(1)) != p0);
    CHECK(t.c.entries.size() == 3 && t.c.n.n_index_reuses == 1 && t.n_closed() == 0);
    std::printf("ok keys\n");
}

static void identity(const std::string &dir)
{
    Bench t; std::string err;
    CHECK(t.c.begin(2, err));
    const ResidentKey k = key("/ref", "0");
    ResidentIdent cur = ident(1);
    int pid = t.call(k, cur);
    uint64_t stale = 0;
    for (int file = 0; file < 4; ++file)
        for (int field = 0; field < 5; ++field) {
            CHECK(t.call(k, cur) == pid && t.c.n.n_stale_reloads == stale);          // unchanged files: found
            FileIdent &f = cur.files[(size_t)file];
            if (field == 0) f.dev += 1; else if (field == 1) f.ino += 1000; else if (field == 2) f.size += 1; else if (field == 3) f.mtime_s += 1; else f.mtime_ns += 1;
            const int before = t.closes_seen;
            const int now = t.call(k, cur);
            CHECK(now != pid && t.c.n.n_stale_reloads == ++stale);
            CHECK(t.closes_seen == before + 1 && t.closed[pid] == 1);                // the stale entry was closed before the call went on
            CHECK(t.c.entries.size() == 1 && t.c.entries[0]->payload.lanes.count(0));   // and the fresh one has the device's lanes
            pid = now;
        }
    CHECK(t.c.n.n_evictions == 0 && t.c.n.n_dropped_after_error == 0);
    // a file that went missing is a change too
    cur.files[2] = FileIdent();
    CHECK(t.call(k, cur) != pid && !cur.complete() && ident(1).complete());
    // real files: rewritten in place, and another file moved over the name
    const std::string pre = dir + "/ix";
    for (const char *ext : RESIDENT_INDEX_FILES) write_file(pre + ext, std::string("first") + ext);
    const ResidentIdent one = resident_ident(pre);
    CHECK(one.complete() && one.files.size() == 4 && one == resident_ident(pre));
    write_file(pre + ".sa", "a longer text than before");
    const ResidentIdent two = resident_ident(pre);
    CHECK(!(two == one) && two.files[2].size != one.files[2].size && two.files[0] == one.files[0]);
    write_file(pre + ".new", std::string("first") + ".bwt");                          // the same size as the file it replaces
    CHECK(::rename((pre + ".new").c_str(), (pre + ".bwt").c_str()) == 0);
    const ResidentIdent three = resident_ident(pre);
    CHECK(!(three == two) && three.files[1].ino != two.files[1].ino && three.files[1].size == two.files[1].size);
    CHECK(::unlink((pre + ".pac").c_str()) == 0);
    CHECK(!resident_ident(pre).complete());
    std::printf("ok identity\n");
}

static void lru(int max_refs)
{
    Bench t; std::string err;
    CHECK(t.c.begin((uint32_t)max_refs, err));
    std::vector<ResidentKey> ks; std::vector<int> pid;
    const int n = max_refs + 3;
    for (int i = 0; i < n; ++i) ks.push_back(key("/ref" + std::to_string(i), i % 2 ? "0,1" : "0"));
    for (int i = 0; i < max_refs; ++i) pid.push_back(t.call(ks[(size_t)i], ident(i)));
    CHECK((int)t.c.entries.size() == max_refs && t.c.n.n_evictions == 0 && t.n_closed() == 0);
    for (int i = 0; i < max_refs; ++i) CHECK(t.call(ks[(size_t)i], ident(i)) == pid[(size_t)i]);      // all found: nothing left
    CHECK(t.c.n.n_index_reuses == (uint64_t)max_refs);
    // touch the oldest: the second oldest is the one to go
    CHECK(t.call(ks[0], ident(0)) == pid[0]);
    const int before = t.closes_seen;
    pid.push_back(t.call(ks[(size_t)max_refs], ident(max_refs)));
    CHECK(t.closes_seen == before + 1 && t.c.n.n_evictions == 1 && (int)t.c.entries.size() == max_refs);
    const int victim = max_refs > 1 ? pid[1] : pid[0];
    CHECK(t.closed[victim] == 1);
    if (max_refs > 1) CHECK(t.call(ks[0], ident(0)) == pid[0]);                                      // still there
    // going round more keys than the scope holds: every call evicts, in order of use
    uint64_t ev = t.c.n.n_evictions;
    for (int round = 0; round < 2; ++round)
        for (int i = 0; i < n; ++i) {
            bool held = false;
            for (auto &e : t.c.entries) held = held || e->key == ks[(size_t)i];
            t.call(ks[(size_t)i], ident(i));
            if (!held) ++ev;
            CHECK(t.c.n.n_evictions == ev && (int)t.c.entries.size() == max_refs);
        }
    CHECK(ev > 1 && t.c.n.n_stale_reloads == 0);
    // a call that uses two entries at once keeps both until it lets go, whatever the bound
    Cache::Entry *a = t.use(ks[0], ident(0)), *b = t.use(ks[1], ident(1));
    CHECK(a != b && a->pinned && b->pinned && t.closed[a->payload.id] == 0 && t.closed[b->payload.id] == 0);
    t.c.release(a); t.c.release(b);
    CHECK((int)t.c.entries.size() == std::min(max_refs, (int)t.c.entries.size()) && (int)t.c.entries.size() <= max_refs);
    t.lanes_ok();
    CHECK(t.c.end(err) && t.c.entries.empty() && t.c.lane_owner.empty());
    CHECK(t.n_closed() == t.next_id);                                  // every entry ever made was closed, once
    std::printf("ok lru %d\n", max_refs);
}

static void drop_and_end()
{
    Bench t; std::string err;
    CHECK(!t.c.end(err) && err.find("no scope is open") != std::string::npos);
    CHECK(t.c.begin(4, err) && !t.c.begin(4, err) && err.find("open already") != std::string::npos);
    const ResidentKey ka = key("/a", "0"), kb = key("/b", "0"), kc = key("/c", "1");
    const int a = t.call(ka, ident(1)), b = t.call(kb, ident(2)), c = t.call(kc, ident(3));
    // a failed call that used a and c: exactly those go, closed before drop returns
    Cache::Entry *ea = t.use(ka, ident(1)), *ec = t.use(kc, ident(3));
    t.c.drop(ea); CHECK(t.closed[a] == 1 && t.closed[c] == 0);
    t.c.drop(ec); CHECK(t.closed[c] == 1 && t.closed[b] == 0);
    CHECK(t.c.n.n_dropped_after_error == 2 && t.c.entries.size() == 1 && t.c.entries[0]->payload.id == b);
    t.lanes_ok();
    CHECK(t.c.lane_owner.empty());                                     // a held device 0's lanes and c device 1's: freed with them
    const int a2 = t.call(ka, ident(1));
    CHECK(a2 != a && t.c.n.n_index_reuses == 2 && t.c.n.n_stale_reloads == 0 && t.c.n.n_evictions == 0);   // loads afresh, counted as neither stale nor evicted
    CHECK(t.call(ka, ident(1), false) == a2 && t.closed[a2] == 1);     // a call that fails on an entry it found
    // ps_index on a path: its entries under every key, and no others
    const int a3 = t.call(ka, ident(1)), a4 = t.call(key("/a", "0,0"), ident(1));
    t.c.invalidate("/a");
    CHECK(t.closed[a3] == 1 && t.closed[a4] == 1 && t.closed[b] == 0 && t.c.entries.size() == 1);
    CHECK(t.c.n.n_dropped_after_error == 3 && t.c.n.n_stale_reloads == 0);
    t.lanes_ok();
    // end closes what is left, the counters stay for ps_resident_info, the next scope starts from zero
    t.call(kc, ident(3));
    const int before = t.closes_seen;
    CHECK(t.c.end(err) && t.closes_seen == before + 2 && t.closed[b] == 1 && t.c.entries.empty() && !t.c.active && t.c.bytes() == 0);
    CHECK(t.c.n.n_dropped_after_error == 3 && t.n_closed() == t.next_id);
    CHECK(t.c.begin(1, err) && t.c.n.n_dropped_after_error == 0 && t.c.n.n_index_reuses == 0 && t.c.max_references == 1);
    CHECK(t.c.end(err));
    std::printf("ok drop_and_end\n");
}

static void lanes()
{
    Bench t; std::string err;
    CHECK(t.c.begin(3, err));
    const ResidentKey g = key("/genome", "0,1"), tr = key("/transcripts", "0,1"), one = key("/genome", "1"), far = key("/far", "2");
    Cache::Entry *e = t.use(g, ident(1));
    CHECK(e->payload.lanes == std::set<int>({0, 1}));
    t.c.release(e);
    e = t.use(tr, ident(2));                                           // takes both devices' lanes over: the genome entry stays, with none
    CHECK(e->payload.lanes == std::set<int>({0, 1}) && t.c.entries[0]->payload.lanes.empty() && t.c.entries.size() == 2);
    t.c.release(e);
    e = t.use(one, ident(1));                                          // device 1 only: device 0's lanes stay where they are
    CHECK(e->payload.lanes == std::set<int>({1}) && t.c.entries[1]->payload.lanes == std::set<int>({0}));
    t.c.release(e);
    e = t.use(far, ident(3));                                          // a fourth entry: the genome entry (the oldest) goes; it held no lanes
    CHECK(t.c.n.n_evictions == 1 && e->payload.lanes == std::set<int>({2}) && t.c.entries.size() == 3);
    t.c.release(e);
    e = t.use(g, ident(1));                                            // back: evicts the transcripts entry, whose device-0 lanes it inherits, and takes device 1's
    CHECK(t.c.n.n_evictions == 2 && e->payload.lanes == std::set<int>({0, 1}));
    t.c.release(e);
    // within one call: genome passes, then the transcript pass, as ps_map_route does
    Cache::Entry *a = t.use(g, ident(1)), *b = t.use(tr, ident(2));
    CHECK(b->payload.lanes == std::set<int>({0, 1}) && a->payload.lanes.empty());
    t.c.release(a); t.c.release(b);
    t.lanes_ok();
    // an entry that is dropped takes the lanes it holds with it; the next call makes new ones
    e = t.use(tr, ident(2)); t.c.drop(e);
    CHECK(!t.c.lane_owner.count(0) && !t.c.lane_owner.count(1));
    t.lanes_ok();
    e = t.use(g, ident(1)); CHECK(e->payload.lanes == std::set<int>({0, 1})); t.c.release(e);
    CHECK(t.c.end(err) && t.n_closed() == t.next_id);
    std::printf("ok lanes\n");
}

static void opts()
{
    ps_resident_opts o, r; std::string err;
    CHECK(resident_opts_read(nullptr, r, err) && r.max_references == 2 && r.struct_size == sizeof(ps_resident_opts));
    o.struct_size = 4; o.max_references = 99;                          // a caller with the size field alone: the default
    CHECK(resident_opts_read(&o, r, err) && r.max_references == 2);
    for (uint32_t m = 1; m <= 8; ++m) { o.struct_size = 8; o.max_references = m; CHECK(resident_opts_read(&o, r, err) && r.max_references == m); }
    for (uint32_t m : {0u, 9u, 0xffffffffu}) { o.struct_size = 8; o.max_references = m; CHECK(!resident_opts_read(&o, r, err) && err.find("max_references") != std::string::npos && err.find("1 to 8") != std::string::npos); }
    for (uint32_t sz : {0u, 2u, 6u, 12u, 64u}) { o.struct_size = sz; o.max_references = 2; CHECK(!resident_opts_read(&o, r, err) && err.find("struct_size") != std::string::npos); }
    std::printf("ok opts\n");
}

int main(int argc, char **argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "keys" && argc > 2) keys(argv[2]);
    else if (what == "identity" && argc > 2) identity(argv[2]);
    else if (what == "lru" && argc > 2) lru(std::atoi(argv[2]));
    else if (what == "drop_and_end") drop_and_end();
    else if (what == "lanes") lanes();
    else if (what == "opts") opts();
    else { std::printf("usage: resident_check keys DIR | identity DIR | lru N | drop_and_end | lanes | opts\n"); return 2; }
    return 0;
}
