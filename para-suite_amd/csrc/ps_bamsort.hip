// ps_bamsort.hip -- the coordinate sort of BAM records and the gather of the sorted stream on the device: what ps_bam.cpp's sort
// hands over when the switch is on (ps_bam_sort_device, PS_BAM_SORT_GPU), and ps_bam_sort_records.  The parts' bytes go up back to
// back through page-locked staging (two halves: one is filled while the other is on the wire), with ref, pos, length and source offset
// per record.  k_bamsort_keys makes ps_bamsort.h's key and the identity; hipcub's radix sort (stable, least significant digit first)
// orders (key, index) over the bits that any key has set; k_bamsort_lens and an exclusive sum give every record of the sorted order
// its destination; k_bamsort_gather -- ps_bamsort.h's group, one wave per 64 consecutive records -- moves the bytes.  The permutation
// comes down at 4 bytes per record, the stream through the same staging -- unless the caller can do without it and the BGZF switch
// names the same device: then the stream stays where it is and ps_bgzf.hip's compressor reads it there (resident_blocks).  No
// workgroup waits for another.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#define PS_BS_DEVICE
#include "ps_bamsort.h"
#include "ps_bgzf.h"
#include "ps_dev.h"
#include "ps_pipeline.h"

namespace ps {

static_assert(BS_STAGE % 16 == 0 && 2 * sizeof(BsShared) <= 64 * 1024, "k_bamsort_gather: static LDS, at least two workgroups in 64 KB");

__global__ __launch_bounds__(256) void k_bamsort_keys(const int32_t *ref, const int32_t *pos, uint64_t n, uint64_t *key, uint32_t *idx)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    key[i] = bamsort_key(ref[i], pos[i]); idx[i] = (uint32_t)i;
}

// lengths in sorted order, n + 1 of them (the last is zero: the exclusive sum then ends with the total)
__global__ __launch_bounds__(256) void k_bamsort_lens(const uint32_t *perm, const uint32_t *len, uint64_t n, uint64_t *slen)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    slen[i] = i < n ? len[perm[i]] : 0;
}

// one wave (= one workgroup) per 64 consecutive records of the sorted order
__global__ __launch_bounds__(BS_NL) void k_bamsort_gather(BsArgs a)
{
    __shared__ BsShared sh;
    bamsort_gather_group(sh, a, (uint64_t)blockIdx.x * BS_NL);
}

namespace {

const size_t PIECE = (size_t)64 << 20;              // one half of the page-locked staging

template <class T> void need(DevBuf<T> &b, size_t n) { if (b.n < n) b.alloc(n); }

struct Buffers {                                    // grow-only, kept between calls (never destroyed: a writer may run during exit)
    int device = -1;
    DevBuf<uint8_t> src, out; DevBuf<uint64_t> off, key_a, key_b, slen, doff; DevBuf<uint32_t> len, idx_a, idx_b; DevBuf<int32_t> ref, pos;
    PinBuf pin;
    void release() { src.release(); out.release(); off.release(); key_a.release(); key_b.release(); slen.release(); doff.release(); len.release(); idx_a.release(); idx_b.release(); ref.release(); pos.release(); }
    void release_host() { if (pin.p) pin_cache_give(pin.p, pin.bytes); pin.p = nullptr; pin.bytes = 0; }
};
std::mutex g_mu;
Buffers &buffers() { static Buffers *b = new Buffers(); return *b; }
std::atomic<int> g_device{-1};
struct Totals { std::mutex mu; BamSortStats s; };
Totals &totals() { static Totals *t = new Totals(); return *t; }

void check_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw Error("ps_bam_sort: no HIP device available");
    if (device < 0 || device >= n) throw Error("ps_bam_sort: no HIP device " + std::to_string(device) + " (" + std::to_string(n) + " present)");
}

void copy_threads(void *dst, const void *src, size_t n)
{
    ranges(n, n >= ((size_t)4 << 20) ? 8 : 1, [&](size_t a0, size_t a1) { std::memcpy((char *)dst + a0, (const char *)src + a0, a1 - a0); });
}

// the two halves of the staging: half() waits until the copy that last used the half is over, sent() marks the one just enqueued
struct Stager {
    uint8_t *base; hipStream_t s; hipEvent_t ev[2] = {nullptr, nullptr}; bool used[2] = {false, false}; int cur = 0;
    Stager(uint8_t *pin, hipStream_t stream) : base(pin), s(stream)
    {
        PS_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
        if (hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) != hipSuccess) { (void)hipEventDestroy(ev[0]); throw Error("hipEventCreate failed"); }
    }
    Stager(const Stager &) = delete;
    ~Stager() { (void)hipStreamSynchronize(s); (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]); }
    uint8_t *half() { if (used[cur]) { PS_HIP(hipEventSynchronize(ev[cur])); used[cur] = false; } return base + (size_t)cur * PIECE; }
    void sent() { PS_HIP(hipEventRecord(ev[cur], s)); used[cur] = true; cur ^= 1; }
    void wait_all() { PS_HIP(hipStreamSynchronize(s)); used[0] = used[1] = false; }
};

uint64_t max_device_bytes()
{
    long long mb = 32768;
    if (const char *e = std::getenv("PS_BAM_SORT_MAX_MB")) if (e[0]) mb = std::atoll(e);
    return mb < 0 ? 0 : (uint64_t)mb << 20;
}

void count(const BamSortStats &x)
{
    Totals &t = totals(); std::lock_guard<std::mutex> l(t.mu);
    t.s.n_records += x.n_records; t.s.bytes += x.bytes; t.s.n_calls_device += x.n_calls_device; t.s.n_calls_host += x.n_calls_host; t.s.n_resident += x.n_resident;
    t.s.ms_upload += x.ms_upload; t.s.ms_sort += x.ms_sort; t.s.ms_gather += x.ms_gather; t.s.ms_download += x.ms_download;
}

// The sorted stream of one call that stayed on the device, between the sort and the compression of its blocks: the buffer is taken
// out of the grow-only set for that time (another thread's sort gets its own) and goes back afterwards.  One at a time: a second call
// that finds the slot taken brings its stream down as usual.
struct Resident { std::mutex mu; bool busy = false; DevBuf<uint8_t> out; uint64_t bytes = 0; int device = -1; };
Resident &resident() { static Resident *r = new Resident(); return *r; }
void resident_blocks(std::string *comp)
{
    Resident &r = resident();
    struct GiveBack {
        Resident &r;
        ~GiveBack()
        {
            {
                std::lock_guard<std::mutex> lock(g_mu);
                Buffers &b = buffers();
                int before = -1; (void)hipGetDevice(&before);
                if (hipSetDevice(r.device) == hipSuccess) { if (b.device == r.device && b.out.n < r.out.n) b.out = std::move(r.out); else r.out.release(); }
                if (before >= 0) (void)hipSetDevice(before);
            }
            std::lock_guard<std::mutex> l(r.mu); r.busy = false; r.bytes = 0;
        }
    } give{r};
    if (comp) bgzf_device_compress_resident(r.out.p, r.bytes, r.device, comp, nullptr);
}

bool device_hook(BamSortJob &job) { return bam_sort_device_run(job, g_device, nullptr); }

// PS_BAM_SORT_GPU=<device>: read once, when the library is loaded; a device that is not there fails the first sorting call
[[maybe_unused]] const bool g_env_read = [] {
    const char *e = std::getenv("PS_BAM_SORT_GPU");
    if (e && e[0]) { const int d = std::atoi(e); if (d >= 0) { g_device = d; bam_sort_set_device_hook(&device_hook); } }
    return true;
}();

}  // namespace

void bam_sort_set_device(int device)
{
    if (device >= 0) check_device(device);
    { Totals &t = totals(); std::lock_guard<std::mutex> l(t.mu); t.s = BamSortStats(); }
    if (device < 0) {                               // switched off: the buffers go back too (a later ps_bam_sort_records takes its own again)
        bam_sort_set_device_hook(nullptr); g_device = -1;
        std::lock_guard<std::mutex> lock(g_mu);
        Buffers &b = buffers();
        if (b.device >= 0) { int before = -1; (void)hipGetDevice(&before); if (hipSetDevice(b.device) == hipSuccess) b.release(); if (before >= 0) (void)hipSetDevice(before); b.device = -1; }
        b.release_host();
        return;
    }
    g_device = device;
    bam_sort_set_device_hook(&device_hook);
}

void bam_sort_info(BamSortStats &out)
{
    Totals &t = totals(); std::lock_guard<std::mutex> l(t.mu);
    out = t.s; out.on_device = g_device >= 0;
}

bool bam_sort_device_run(BamSortJob &job, int device, BamSortStats *stats)
{
    BamSortStats st;
    const size_t n = job.n_recs;
    // ---- what the call needs, before any device call: source offsets of the parts, the records inside them, the device memory
    std::vector<uint64_t> base(job.n_parts + 1, 0);
    for (size_t k = 0; k < job.n_parts; ++k) base[k + 1] = base[k] + job.parts[k].n;
    const uint64_t src_bytes = base[job.n_parts];
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        const BamRec &r = job.recs[i];
        if (r.part < 0 || (size_t)r.part >= job.n_parts || r.len > 0xffffffffull || r.off > job.parts[r.part].n || r.len > job.parts[r.part].n - r.off)
            throw Error("ps_bam_sort: record " + std::to_string(i + 1) + " lies outside its buffer");
        total += r.len;
    }
    const uint64_t device_bytes = src_bytes + total + 64 * (uint64_t)n + ((uint64_t)32 << 20);
    if (n >= ((uint64_t)1 << 32) || device_bytes > max_device_bytes()) {
        st.n_calls_host = 1; count(st);
        if (stats) *stats = st;
        return false;
    }
    st.on_device = 1; st.n_calls_device = 1; st.n_records = n; st.bytes = total;
    job.resident = nullptr;
    bool stay = false;
    if (n && job.may_stay && bgzf_device_current() == device) { Resident &r = resident(); std::lock_guard<std::mutex> l(r.mu); if (!r.busy) { r.busy = true; stay = true; } }
    struct Unbusy { bool armed; ~Unbusy() { if (armed) { Resident &r = resident(); std::lock_guard<std::mutex> l(r.mu); r.busy = false; } } } unbusy{stay};   // an error on the way
    job.perm->assign(n, 0); job.stream->assign(stay ? 0 : (size_t)total, '\0');
    if (n == 0) { count(st); if (stats) *stats = st; return true; }

    std::lock_guard<std::mutex> lock(g_mu);
    check_device(device);
    DeviceScope scope(device);
    Buffers &b = buffers();
    if (b.device != device) { b.release(); b.device = device; }
    need(b.src, (size_t)((src_bytes + 3) & ~(uint64_t)3) + 16); need(b.out, (size_t)total + 16);
    need(b.off, n); need(b.len, n); need(b.ref, n); need(b.pos, n);
    need(b.key_a, n); need(b.key_b, n); need(b.idx_a, n); need(b.idx_b, n); need(b.slen, n + 1); need(b.doff, n + 1);
    uint8_t *pin = (uint8_t *)b.pin.get(2 * PIECE);
    StreamGuard sg;
    Stager stg(pin, sg.s);

    // ---- upload: the parts back to back, then the four columns, piece by piece
    HostClock::time_point t0 = HostClock::now();
    {
        size_t k = 0; uint64_t in_part = 0, at = 0;
        while (at < src_bytes) {
            uint8_t *h = stg.half();
            size_t fill = 0;
            while (fill < PIECE && k < job.n_parts) {
                const size_t take = (size_t)std::min<uint64_t>(PIECE - fill, job.parts[k].n - in_part);
                if (take) copy_threads(h + fill, job.parts[k].p + in_part, take);
                fill += take; in_part += take;
                if (in_part == job.parts[k].n) { ++k; in_part = 0; }
            }
            PS_HIP(hipMemcpyAsync(b.src.p + at, h, fill, hipMemcpyHostToDevice, sg.s));
            stg.sent();
            at += fill;
        }
    }
    uint64_t any = 0;
    {
        const size_t per = PIECE / 20;              // off 8, len 4, ref 4, pos 4 per record
        for (size_t i0 = 0; i0 < n; i0 += per) {
            const size_t m = std::min(per, n - i0);
            uint8_t *h = stg.half();
            uint64_t *h_off = (uint64_t *)h; uint32_t *h_len = (uint32_t *)(h + 8 * per); int32_t *h_ref = (int32_t *)(h + 12 * per), *h_pos = (int32_t *)(h + 16 * per);
            std::atomic<uint64_t> any_piece{0};
            ranges(m, m >= 65536 ? 8 : 1, [&](size_t a0, size_t a1) {
                uint64_t o = 0;
                for (size_t j = a0; j < a1; ++j) {
                    const BamRec &r = job.recs[i0 + j];
                    h_off[j] = base[(size_t)r.part] + r.off; h_len[j] = (uint32_t)r.len; h_ref[j] = r.ref; h_pos[j] = r.pos;
                    o |= bamsort_key(r.ref, r.pos);
                }
                any_piece |= o;
            });
            any |= any_piece.load();
            PS_HIP(hipMemcpyAsync(b.off.p + i0, h_off, m * 8, hipMemcpyHostToDevice, sg.s));
            PS_HIP(hipMemcpyAsync(b.len.p + i0, h_len, m * 4, hipMemcpyHostToDevice, sg.s));
            PS_HIP(hipMemcpyAsync(b.ref.p + i0, h_ref, m * 4, hipMemcpyHostToDevice, sg.s));
            PS_HIP(hipMemcpyAsync(b.pos.p + i0, h_pos, m * 4, hipMemcpyHostToDevice, sg.s));
            stg.sent();
        }
    }
    stg.wait_all();
    st.ms_upload = ms_since(t0); t0 = HostClock::now();

    // ---- keys, the sort over the bits that any key has set (all placed: 32 + the bits of the largest reference id)
    const int end_bit = bamsort_end_bit(any);
    hipLaunchKernelGGL(k_bamsort_keys, dim3(blocks_for(n)), dim3(256), 0, sg.s, b.ref.p, b.pos.p, (uint64_t)n, b.key_a.p, b.idx_a.p);
    PS_HIP(hipGetLastError());
    cub_call(sg.s, [&](void *tmp, size_t &bytes) { return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, b.key_a.p, b.key_b.p, b.idx_a.p, b.idx_b.p, n, 0, end_bit, sg.s); });
    st.ms_sort = ms_since(t0); t0 = HostClock::now();

    // ---- destinations, then the bytes
    hipLaunchKernelGGL(k_bamsort_lens, dim3(blocks_for(n + 1)), dim3(256), 0, sg.s, b.idx_b.p, b.len.p, (uint64_t)n, b.slen.p);
    PS_HIP(hipGetLastError());
    cub_call(sg.s, [&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, b.slen.p, b.doff.p, n + 1, sg.s); });
    uint64_t d_total = 0;
    PS_HIP(hipMemcpyAsync(&d_total, b.doff.p + n, sizeof d_total, hipMemcpyDeviceToHost, sg.s));
    PS_HIP(hipStreamSynchronize(sg.s));
    if (d_total != total) throw Error("ps_bam_sort: the device's offsets do not end at the records' size");
    BsArgs a{b.src.p, b.off.p, b.len.p, b.idx_b.p, b.doff.p, (uint64_t)n, b.out.p};
    hipLaunchKernelGGL(k_bamsort_gather, dim3((unsigned)((n + BS_NL - 1) / BS_NL)), dim3(BS_NL), 0, sg.s, a);
    PS_HIP(hipGetLastError());
    PS_HIP(hipStreamSynchronize(sg.s));
    st.ms_gather = ms_since(t0); t0 = HostClock::now();

    // ---- the permutation and the stream come down; a half is copied out while the next piece is on the wire
    {
        struct Piece { uint8_t *h; char *dst; size_t bytes; };
        Piece prev{nullptr, nullptr, 0};
        auto down = [&](const uint8_t *d_src, char *dst, size_t bytes) {
            for (size_t at = 0; at < bytes; at += PIECE) {
                const size_t m = std::min(PIECE, bytes - at);
                uint8_t *h = stg.half();
                PS_HIP(hipMemcpyAsync(h, d_src + at, m, hipMemcpyDeviceToHost, sg.s));
                stg.sent();
                if (prev.h) { PS_HIP(hipEventSynchronize(stg.ev[stg.cur])); stg.used[stg.cur] = false; copy_threads(prev.dst, prev.h, prev.bytes); }   // cur names the other half again: the one sent before
                prev = Piece{h, dst + at, m};
            }
        };
        down((const uint8_t *)b.idx_b.p, (char *)job.perm->data(), n * sizeof(uint32_t));
        if (!stay) down(b.out.p, &(*job.stream)[0], (size_t)total);
        stg.wait_all();
        if (prev.h) copy_threads(prev.dst, prev.h, prev.bytes);
    }
    st.ms_download = ms_since(t0);
    if (stay) {                                     // the stream's buffer leaves the set until its blocks are made
        Resident &r = resident();
        r.out = std::move(b.out); r.bytes = total; r.device = device;
        unbusy.armed = false;
        job.resident = &resident_blocks;
        st.n_resident = 1;
    }
    count(st);
    if (stats) *stats = st;
    static const bool verbose = std::getenv("PS_VERBOSE") != nullptr;
    if (verbose)
        std::fprintf(stderr, "[parasuite-hip] bam sort: %zu records, %.1f MB on device %d: upload %.1f ms, keys + sort over %d bits %.1f ms, offsets + gather %.1f ms, download %.1f ms%s\n",
                     n, total / 1e6, device, st.ms_upload, end_bit, st.ms_sort, st.ms_gather, st.ms_download, stay ? " (the permutation alone: the stream stays for the compressor)" : "");
    return true;
}

}  // namespace ps
