// ps_resident.h -- the book-keeping of the resident scope (include/parasuite_hip.h: ps_resident_begin / _end / _info): which
// indexes a process keeps in HBM between its mapping calls, under which key, and which of them holds a device's lanes of work.
// Host only, no HIP and no call into the library: what an entry holds is a template parameter (ps_map.hip: the CtxSet of a pass)
// and closing it is a function handed in, so tests/resident_check.cpp drives this header alone with stub closers.
// Not thread safe: ps_map.hip calls it under its own lock.
#pragma once
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include <sys/stat.h>
#include "../../include/parasuite_hip.h"
#include "ps_map_plan.h"

namespace ps {

// the caller's struct as this library's, by the rules of ps_search_opts (ps_search_opts.h): the fields behind the caller's
// struct_size keep their defaults, a size that is no whole number of fields or larger than this library knows is refused
inline bool resident_opts_read(const ps_resident_opts *in, ps_resident_opts &o, std::string &err)
{
    o.struct_size = (uint32_t)sizeof(ps_resident_opts); o.max_references = 2;
    if (in) {
        const uint32_t sz = in->struct_size;
        if (sz < sizeof(uint32_t) || sz % sizeof(uint32_t) != 0 || sz > sizeof(ps_resident_opts)) {
            err = "ps_resident_opts: struct_size " + std::to_string(sz) + " must be a multiple of 4 from 4 to " + std::to_string(sizeof(ps_resident_opts));
            return false;
        }
        std::memcpy(&o, in, sz);
        o.struct_size = (uint32_t)sizeof(ps_resident_opts);
    }
    if (o.max_references < 1 || o.max_references > 8) {
        err = "ps_resident_opts: max_references is " + std::to_string(o.max_references) + ", accepted: 1 to 8";
        return false;
    }
    return true;
}

// The knobs that shape what is resident (the depth of the jump table, the size of the search workspace), as the code that acts on
// them read them: an entry made under other values is another entry.
struct ResidentKnobs { int jump = 1, jump_levels = -1, pool_cap = 0, n_big = 0, bt_blocks = 0; };   // PS_JUMP (0: off), PS_JUMP_LEVELS (-1: not stated), PS_POOL_CAP, PS_N_BIG, PS_BT_BLOCKS
inline uint64_t resident_fingerprint(const ResidentKnobs &k)
{
    uint64_t h = 0xcbf29ce484222325ull;                          // FNV-1a over the five values
    for (int v : {k.jump, k.jump_levels, k.pool_cap, k.n_big, k.bt_blocks})
        for (int b = 0; b < 4; ++b) { h ^= (uint64_t)(((uint32_t)v >> (8 * b)) & 0xffu); h *= 0x100000001b3ull; }
    return h;
}

// the reference as realpath names it; a prefix with index files but no FASTA beside them goes by its .ann file; what cannot be
// resolved stays as it was spelled
inline std::string resident_path(const char *ref)
{
    const std::string given = ref ? ref : "";
    char buf[PATH_MAX];
    if (::realpath(given.c_str(), buf)) return buf;
    if (::realpath((given + ".ann").c_str(), buf)) { std::string s = buf; return s.substr(0, s.size() - 4); }
    return given;
}

struct ResidentKey {
    std::string path; std::vector<int> devs, workers; uint64_t knobs = 0;
    bool operator==(const ResidentKey &o) const { return path == o.path && devs == o.devs && workers == o.workers && knobs == o.knobs; }
};
inline ResidentKey resident_key(const char *ref, const DevicePlan &plan, const ResidentKnobs &knobs)
{
    ResidentKey k; k.path = resident_path(ref); k.devs = plan.devs; k.workers = plan.workers; k.knobs = resident_fingerprint(knobs);
    return k;
}

// what tells one version of an index file from the next
struct FileIdent {
    uint64_t dev = 0, ino = 0; int64_t size = -1, mtime_s = 0, mtime_ns = 0;              // size -1: no such file
    bool operator==(const FileIdent &o) const { return dev == o.dev && ino == o.ino && size == o.size && mtime_s == o.mtime_s && mtime_ns == o.mtime_ns; }
};
inline FileIdent file_ident(const struct stat &st)
{
    FileIdent f; f.dev = (uint64_t)st.st_dev; f.ino = (uint64_t)st.st_ino; f.size = (int64_t)st.st_size;
    f.mtime_s = (int64_t)st.st_mtim.tv_sec; f.mtime_ns = (int64_t)st.st_mtim.tv_nsec;
    return f;
}
struct ResidentIdent {
    std::vector<FileIdent> files;
    bool operator==(const ResidentIdent &o) const { return files == o.files; }
    bool complete() const { for (const FileIdent &f : files) if (f.size < 0) return false; return !files.empty(); }
};
static const char *const RESIDENT_INDEX_FILES[] = {".ann", ".bwt", ".sa", ".pac"};      // the files index_load opens
inline ResidentIdent resident_ident(const std::string &prefix)
{
    ResidentIdent id;
    for (const char *ext : RESIDENT_INDEX_FILES) {
        struct stat st;
        id.files.push_back(::stat((prefix + ext).c_str(), &st) == 0 ? file_ident(st) : FileIdent());
    }
    return id;
}

struct ResidentCounters { uint64_t n_calls = 0, n_index_loads = 0, n_index_reuses = 0, n_stale_reloads = 0, n_evictions = 0, n_dropped_after_error = 0; };

// The entries of a scope.  P: what an entry holds.  close(gone, heir) gives back everything `gone` holds before it returns; where
// `heir` is not null it is the entry made in the same step, which takes over the lanes of work of the devices the two share.
// A device has one set of lanes whatever the number of entries: lane_owner names the entry whose payload holds them, and a call
// that is about to use another entry moves them (take_lanes) instead of making a second set.
template <class P> struct ResidentCache {
    struct Entry { ResidentKey key; ResidentIdent id; P payload; uint64_t used = 0, bytes = 0; bool pinned = false, fresh = true; };
    std::function<void(P &gone, P *heir)> close;
    bool active = false; uint32_t max_references = 2; ResidentCounters n; uint64_t tick = 0;
    std::vector<std::unique_ptr<Entry>> entries;
    std::map<int, Entry *> lane_owner;

    bool begin(uint32_t max_refs, std::string &err)
    {
        if (active) { err = "ps_resident_begin: a scope is open already (ps_resident_end closes it)"; return false; }
        active = true; max_references = max_refs; n = ResidentCounters(); tick = 0;
        return true;
    }
    bool end(std::string &err)
    {
        if (!active) { err = "ps_resident_end: no scope is open"; return false; }
        while (!entries.empty()) remove(oldest(true), nullptr);
        active = false;
        return true;
    }
    uint64_t bytes() const { uint64_t b = 0; for (const auto &e : entries) b += e->bytes; return b; }

    // The entry of a call, pinned until release() or drop().  An entry with the key whose files are no longer the ones it was
    // loaded from is closed and made afresh; so is, when the scope holds max_references already, the least recently used one that
    // no call has pinned.  make(payload) fills a fresh entry before anything is closed, so that it can inherit lanes.
    Entry *acquire(const ResidentKey &k, const ResidentIdent &id, const std::function<void(P &)> &make)
    {
        ++tick;
        Entry *old = nullptr;
        for (auto &e : entries) if (e->key == k) old = e.get();
        if (old && old->id == id) { old->used = tick; old->pinned = true; old->fresh = false; ++n.n_index_reuses; return old; }
        entries.emplace_back(new Entry());
        Entry *e = entries.back().get();
        e->key = k; e->id = id; e->used = tick; e->pinned = true;
        if (make) make(e->payload);
        if (old) { ++n.n_stale_reloads; remove(old, e); }
        trim(e);
        return e;
    }
    // the entries whose payloads hold lanes of work on e's devices, which now become e's: the caller moves them
    std::vector<Entry *> take_lanes(Entry *e)
    {
        std::vector<Entry *> from;
        for (int d : e->key.devs) {
            auto it = lane_owner.find(d);
            if (it != lane_owner.end() && it->second != e) {
                bool seen = false;
                for (Entry *f : from) seen = seen || f == it->second;
                if (!seen) from.push_back(it->second);
            }
            lane_owner[d] = e;
        }
        return from;
    }
    void release(Entry *e) { e->pinned = false; trim(nullptr); }           // a call that ended well: the entry stays
    void drop(Entry *e) { ++n.n_dropped_after_error; remove(e, nullptr); trim(nullptr); }   // a call that failed: the next one loads afresh
    void invalidate(const std::string &path)                              // the index files of `path` are about to be written
    {
        for (size_t i = entries.size(); i-- > 0;) if (entries[i]->key.path == path) remove(entries[i].get(), nullptr);
    }

private:
    Entry *oldest(bool pinned_too)
    {
        Entry *o = nullptr;
        for (auto &e : entries) if ((pinned_too || !e->pinned) && (!o || e->used < o->used)) o = e.get();
        return o;
    }
    void trim(Entry *heir)
    {
        while (entries.size() > max_references) {
            Entry *o = oldest(false);
            if (!o) return;                                              // all in use by the running call: trimmed when it lets go
            ++n.n_evictions; remove(o, heir);
        }
    }
    void remove(Entry *e, Entry *heir)
    {
        bool inherits = false;
        for (auto it = lane_owner.begin(); it != lane_owner.end();) {
            if (it->second != e) { ++it; continue; }
            bool shared = false;
            if (heir) for (int d : heir->key.devs) shared = shared || d == it->first;
            if (shared) { it->second = heir; inherits = true; ++it; } else it = lane_owner.erase(it);
        }
        if (close) close(e->payload, inherits ? &heir->payload : nullptr);
        for (size_t i = 0; i < entries.size(); ++i) if (entries[i].get() == e) { entries.erase(entries.begin() + (long)i); break; }
    }
};

}  // namespace ps
