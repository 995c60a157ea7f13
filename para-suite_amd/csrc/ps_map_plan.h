// ps_map_plan.h -- the parts of the streaming map pass (ps_map.hip) with no device in them: which devices and how many workers,
// how large the pieces, and the bounded hand-over between the stages.  Nothing from HIP is included: tests/test_map_plan_cpu.py
// builds this header alone.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <vector>

namespace ps {

// bounded hand-over between the stages of ps_map
template <class T> struct Chan {
    std::mutex m; std::condition_variable cv; std::deque<T> q; bool closed = false; size_t cap = 2; int waiting = 0;
    void push(T &&v) { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return q.size() < cap || closed; }); if (closed) return; q.push_back(std::move(v)); cv.notify_all(); }
    bool pop(T &v) { std::unique_lock<std::mutex> l(m); ++waiting; cv.wait(l, [&] { return !q.empty() || closed; }); --waiting; if (q.empty()) return false; v = std::move(q.front()); q.pop_front(); cv.notify_all(); return true; }
    bool hungry() { std::lock_guard<std::mutex> l(m); return q.empty() && waiting > 0; }     // somebody waits for work and there is none
    void close() { std::lock_guard<std::mutex> l(m); closed = true; cv.notify_all(); }      // what is queued is still handed out
    void abort() { std::lock_guard<std::mutex> l(m); closed = true; q.clear(); cv.notify_all(); }
};

// Devices: the first `gpus_wanted` of the `devices_present` (PARASUITE_GPUS, default 1), or the comma-separated list `ids`
// (PARASUITE_GPU_IDS).  Every device has `per_dev` workers (PS_WORKERS_PER_GPU, default 1), a device named twice gets two, and none
// more than `max_lanes` (Ctx::N_WORK: a worker is a lane of work of the device's context).
struct DevicePlan {
    std::vector<int> devs, workers;                  // distinct devices in the order named; workers on each
    int n_workers() const { int n = 0; for (int w : workers) n += w; return n; }
};
inline DevicePlan plan_devices(const char *ids, int gpus_wanted, int per_dev, int devices_present, int max_lanes)
{
    std::vector<int> named;
    if (ids) { for (const char *p = ids; *p;) { named.push_back(std::atoi(p)); while (*p && *p != ',') ++p; if (*p == ',') ++p; } }
    else for (int g = 0; g < std::min(std::max(1, gpus_wanted), devices_present); ++g) named.push_back(g);
    if (named.empty()) named.push_back(0);
    DevicePlan d;
    for (int dev : named) {
        size_t k = 0;
        while (k < d.devs.size() && d.devs[k] != dev) ++k;
        if (k == d.devs.size()) { d.devs.push_back(dev); d.workers.push_back(0); }
        ++d.workers[k];
    }
    for (int &w : d.workers) w = std::min(max_lanes, std::max(w, std::max(1, per_dev)));
    return d;
}

// Piece size from the input.
// Few, large pieces: every search launch ends with its longest read (~0.25 s of a launch are that, whatever its size: a 1.25 M-read
// launch takes 0.37 s, 10 M reads in one 1.1 s).  The parser hands over what it has when a worker WAITS for work (the first piece
// as soon as the index is resident) but not less than 20 % of the input (hungry_min), and otherwise lets a piece grow to 1 GB
// (chunk_bytes); with several workers a piece is at most 1/(2 x workers) of the input, so that all of them get some.
// file_bytes 0: size unknown (no file, or reads already in memory).  The stated values are MB, 0 = not stated: PS_CHUNK_MB is taken
// as it is (and is the hungry size too), PS_HUNGRY_MIN_MB and PS_FIRST_MB (the first piece; the following ones double up to the
// piece size) override what the size gave.
struct PiecePlan { size_t chunk_bytes, hungry_min, first_bytes; };
inline PiecePlan plan_pieces(size_t file_bytes, int n_workers, bool bam_out, int stated_chunk_mb, int stated_hungry_mb, int stated_first_mb)
{
    PiecePlan p{(size_t)1 << 30, (size_t)128 << 20, 0};
    const size_t sz = file_bytes, nw = (size_t)n_workers;
    if (stated_chunk_mb > 0) p.hungry_min = p.chunk_bytes = (size_t)stated_chunk_mb << 20;
    else if (sz > 0) {
        if (nw > 1) p.chunk_bytes = std::min(p.chunk_bytes, std::max<size_t>((size_t)16 << 20, (sz + 2 * nw - 1) / (2 * nw) + ((size_t)64 << 10)));   // + slack: cuts fall behind whole records, the last piece must not be a few reads
        p.hungry_min = std::min(p.chunk_bytes, std::max(p.hungry_min, sz / 5));
        // BAM out: compressing the records (2.3 s per 10 M reads at zlib level 1, 16 threads) is the slowest stage and can only
        // start on a piece the GPU has finished -- four pieces, so that it starts early (3.5 -> 3.0 s per 10 M reads)
        if (bam_out) { p.chunk_bytes = std::min(p.chunk_bytes, std::max<size_t>((size_t)64 << 20, sz / 4 + ((size_t)64 << 10))); p.hungry_min = std::min(p.hungry_min, p.chunk_bytes / 2); }
    }
    if (stated_hungry_mb > 0) p.hungry_min = (size_t)stated_hungry_mb << 20;
    if (stated_first_mb > 0) p.first_bytes = (size_t)stated_first_mb << 20;
    return p;
}

}  // namespace ps
