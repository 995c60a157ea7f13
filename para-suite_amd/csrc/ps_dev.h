// ps_dev.h -- what the host code of every analysis mode does around its kernels (ps_profile, ps_clusters, ps_combine,
// ps_benchmark; the clock and the event timer serve the mapping stages too): a stream of its own, tables onto the device, a hipCUB call, times, the reference's tables (a text file: ps_outfiles.h).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <map>
#include <thread>
#include "ps_host.h"
#include "ps_bam.h"
#include "ps_outfiles.h"

namespace ps {

struct StreamGuard {                   // a non-blocking stream; waited for, then destroyed
    hipStream_t s = nullptr;
    StreamGuard() { PS_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    StreamGuard(const StreamGuard &) = delete;
    ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
};

// an empty table still gets one element: no kernel is handed a null pointer
template <class T> void upload(DevBuf<T> &d, const std::vector<T> &v, hipStream_t s)
{
    d.alloc(std::max<size_t>(1, v.size()));
    if (!v.empty()) d.upload(v.data(), v.size(), s);
}

template <class F> void cub_call(hipStream_t s, F f)       // f(temporary storage, its size): the size query, then the call, waited for
{
    size_t bytes = 0;
    PS_HIP(f(nullptr, bytes));
    DevBuf<uint8_t> tmp; tmp.alloc(std::max<size_t>(bytes, 1));
    PS_HIP(f((void *)tmp.p, bytes));
    PS_HIP(hipStreamSynchronize(s));
}
inline unsigned blocks_for(size_t n, unsigned per = 256) { return (unsigned)std::max<size_t>(1, (n + per - 1) / per); }

struct DeviceScope {                                // the calling thread's device, put back on the way out
    int before = -1;
    explicit DeviceScope(int device) { (void)hipGetDevice(&before); PS_HIP(hipSetDevice(device)); }
    DeviceScope(const DeviceScope &) = delete;
    ~DeviceScope() { if (before >= 0) (void)hipSetDevice(before); }
};
struct QuietDeviceScope {                           // the same where the caller must not throw (a destructor, a switch that goes off): ok says whether the device is set
    int before = -1; bool ok = false;
    explicit QuietDeviceScope(int device) noexcept { (void)hipGetDevice(&before); ok = hipSetDevice(device) == hipSuccess; }
    QuietDeviceScope(const QuietDeviceScope &) = delete;
    ~QuietDeviceScope() { if (before >= 0) (void)hipSetDevice(before); }
};
inline void check_device(const char *who, int device)   // throws "<who>: no HIP device ..." unless `device` is one of those present
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw Error(std::string(who) + ": no HIP device available");
    if (device < 0 || device >= n) throw Error(std::string(who) + ": no HIP device " + std::to_string(device) + " (" + std::to_string(n) + " present)");
}

// f(begin, end) over [0, n) on up to `threads` threads
template <class F> void ranges(size_t n, int threads, F f)
{
    const size_t nt = std::min<size_t>((size_t)std::max(1, threads), n);
    if (nt <= 1) { if (n) f((size_t)0, n); return; }
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; ++t) th.emplace_back([&, t]() { f(n * t / nt, n * (t + 1) / nt); });
    for (auto &x : th) x.join();
}

using HostClock = std::chrono::steady_clock;
inline double ms_since(HostClock::time_point t) { return std::chrono::duration<double, std::milli>(HostClock::now() - t).count(); }

struct EventPair {                     // device time between start() and stop() on one stream
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() { PS_HIP(hipEventCreate(&a)); if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); throw Error("hipEventCreate failed"); } }
    explicit EventPair(hipStream_t s) : EventPair() { start(s); }
    EventPair(const EventPair &) = delete;
    ~EventPair() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
    void start(hipStream_t s) { PS_HIP(hipEventRecord(a, s)); }
    void stop(hipStream_t s) { PS_HIP(hipEventRecord(b, s)); }
    // stop(): the end is recorded and the host goes on submitting; ms(): the time, once the host has a reason to wait anyway
    double ms() { PS_HIP(hipEventSynchronize(b)); float v = 0; PS_HIP(hipEventElapsedTime(&v, a, b)); return v; }   // waits for stop()
    // start / stop on a context's clock (ms since its reference event): launches of two streams that overlap in time
    void span(hipEvent_t ref, double &t_begin, double &t_end) { float x = 0, y = 0; if (ref && hipEventElapsedTime(&x, ref, a) == hipSuccess && hipEventElapsedTime(&y, ref, b) == hipSuccess) { t_begin = x; t_end = y; } }
};
// elapsed milliseconds of what `launch` enqueues on s, waited for
template <class F> double timed(hipStream_t s, F launch)
{
    EventPair ev;
    ev.start(s); launch(); ev.stop(s);
    return ev.ms();
}

// the columns of a record table that its mask names (ref, pos, flag and l_seq always), on the device
struct DevRecTable {
    DevBuf<int32_t> ref, pos, l_seq; DevBuf<uint32_t> flag, cig_off, n_cig, cigar;
    DevBuf<uint64_t> seq_off, name_off; DevBuf<uint8_t> seq, qual, name_len, names;
    void upload(const RecTable &t, hipStream_t s)
    {
        ps::upload(ref, t.ref, s); ps::upload(pos, t.pos, s); ps::upload(l_seq, t.l_seq, s); ps::upload(flag, t.flag, s);
        if (t.columns & kRecCigar) { ps::upload(cig_off, t.cig_off, s); ps::upload(n_cig, t.n_cig, s); ps::upload(cigar, t.cigar, s); }
        if (t.columns & (kRecSeq | kRecQual)) ps::upload(seq_off, t.seq_off, s);
        if (t.columns & kRecSeq) ps::upload(seq, t.seq, s);
        if (t.columns & kRecQual) ps::upload(qual, t.qual, s);
        if (t.columns & kRecNames) { ps::upload(name_off, t.name_off, s); ps::upload(name_len, t.name_len, s); ps::upload(names, t.names, s); }
    }
};

// the reference side of a mode that compares records with the index's packed forward strand: per contig its length and its
// offset on that strand, the holes (runs of non-ACGT letters) by offset and length -- on the device, complete on return
struct RefTables {
    DevBuf<int32_t> contig_len, hole_len; DevBuf<int64_t> contig_off, hole_off; int n_holes = 0;
    RefTables(const Index &ix, hipStream_t s)
    {
        std::vector<int32_t> clen, hlen; std::vector<int64_t> coff, hoff;
        for (const Contig &c : ix.ref.contigs) { clen.push_back(c.len); coff.push_back(c.offset); }
        for (const Hole &h : ix.ref.holes) { hoff.push_back(h.offset); hlen.push_back(h.len); }
        n_holes = (int)hoff.size();
        upload(contig_len, clen, s); upload(contig_off, coff, s); upload(hole_off, hoff, s); upload(hole_len, hlen, s);
        PS_HIP(hipStreamSynchronize(s));
    }
    // @SQ entry of a mapping -> contig of the index with that name, -1 where there is none
    static std::vector<int32_t> ref_to_contig(const Index &ix, const std::vector<std::pair<std::string, uint32_t>> &refs)
    {
        std::map<std::string, int> contig_of;
        for (size_t c = 0; c < ix.ref.contigs.size(); ++c) contig_of[ix.ref.contigs[c].name] = (int)c;
        std::vector<int32_t> out(refs.size(), -1);
        for (size_t r = 0; r < refs.size(); ++r) { auto it = contig_of.find(refs[r].first); if (it != contig_of.end()) out[r] = it->second; }
        return out;
    }
};

// beside RefTables, for a mode that writes reference text (ps_fetch): per hole its character, upper-cased -- all the index keeps
// of a hole's text, and with the packed strand all of the FASTA but the case of a, c, g and t
struct RefHoleChars {
    DevBuf<uint8_t> chr;
    RefHoleChars(const Index &ix, hipStream_t s)
    {
        std::vector<uint8_t> c;
        for (const Hole &h : ix.ref.holes) c.push_back((uint8_t)(h.amb >= 'a' && h.amb <= 'z' ? h.amb - 32 : h.amb));
        upload(chr, c, s);
        PS_HIP(hipStreamSynchronize(s));
    }
};

}  // namespace ps
