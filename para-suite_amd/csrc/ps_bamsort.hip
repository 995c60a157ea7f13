// ps_bamsort.hip -- the coordinate sort of BAM records and the gather of the sorted stream on the device: what ps_bam.cpp's sort
// hands over when the switch is on (ps_bam_sort_device, PS_BAM_SORT_GPU), and ps_bam_sort_records.  The parts' bytes go up back to
// back through page-locked staging (two halves: one is filled while the other is on the wire), with ref, pos, length and source offset
// per record.  k_bamsort_keys makes ps_bamsort.h's key and the identity; hipcub's radix sort (stable, least significant digit first)
// orders (key, index) over the bits that any key has set; k_bamsort_lens and an exclusive sum give every record of the sorted order
// its destination; k_bamsort_gather -- ps_bamsort.h's group, one wave per 64 consecutive records -- moves the bytes.  The permutation
// comes down at 4 bytes per record, the stream through the same staging -- unless the caller can do without it and the BGZF switch
// names the same device: then the stream stays where it is and ps_bgzf.hip's compressor reads it there (ResidentStream).  No
// workgroup waits for another.
//
// The name sort (ps_bam_name_sort_device, PS_BAM_NAME_SORT_GPU, ps_bam_name_sort_records) is the same route with another order:
// k_namesort_rows makes ps_namesort.h's row of W words per record, column-major, and the OR and the AND of every column; then, from
// the last column to the first, k_namesort_column fetches the column in the current order and hipcub's stable radix sort orders
// (word, index) over the bits in which the column's words differ -- a column whose words all agree is skipped.  Upload, destinations,
// gather, download and the resident hand-over are run_route's, for both orders.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#define PS_BS_DEVICE
#include "ps_bamsort.h"
#include "ps_namesort.h"
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

// The rows of the name order.  One wave (= one workgroup) per 64 consecutive records of the input.  The lanes stage the group's names
// into LDS -- 16 lanes per name, four names at a time, aligned 4-byte loads realigned in registers (bs_src_word) -- at a stride of
// 65 words, so that lanes reading their own names at equal offsets meet no bank twice.  Then every lane runs the generator over its
// own name: the loop over the W words is the same for the whole wave, and word w of the 64 records is one contiguous store of 256
// bytes.  The OR and the AND of every column are reduced over the wave and go out as one atomic each, and only when they would change
// what is there (both only ever gain or lose bits, so a stale look costs an atomic and never an answer).
__global__ __launch_bounds__(NS_NL) void k_namesort_rows(const uint8_t *src, const uint64_t *rec_off, const int32_t *name_len, const int32_t *pair, uint64_t n, uint32_t W,
                                                         uint32_t *col, uint32_t *col_or, uint32_t *col_and)
{
    __shared__ uint32_t names[NS_NL * NS_NAME_STRIDE];
    __shared__ uint64_t s_off[NS_NL];
    __shared__ uint32_t s_len[NS_NL];
    const uint32_t lane = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * NS_NL + lane;
    const bool live = i < n;
    uint32_t len = live ? (uint32_t)name_len[i] : 0u;
    if (len > NS_MAX_NAME) len = NS_MAX_NAME;                                  // the host has refused such a call; a lane never leaves its row
    s_off[lane] = live ? rec_off[i] + 36 : 0; s_len[lane] = len;
    __syncthreads();
    for (uint32_t r = lane >> 4; r < NS_NL; r += 4) {
        const uint64_t a = s_off[r]; const uint32_t l = s_len[r];
        const int64_t lo = (int64_t)(a & ~(uint64_t)3), hi = (int64_t)((a + l + 3) & ~(uint64_t)3);
        for (uint32_t w = lane & 15; w < ((l + 3) >> 2); w += 16) names[r * NS_NAME_STRIDE + w] = bs_src_word(src, (int64_t)a + 4 * (int64_t)w, lo, hi);
    }
    __syncthreads();
    const uint8_t *name = (const uint8_t *)(names + lane * NS_NAME_STRIDE);
    const uint32_t pr = live ? (uint32_t)pair[i] : 0u;
    NsGen g;
    for (uint32_t w = 0; w < W; ++w) {
        const uint32_t v = namesort_row_word(namesort_next_word(g, name, len), w, W, pr);
        if (live) col[(uint64_t)w * n + i] = v;
        uint32_t o = live ? v : 0u, a = live ? v : ~0u;
        for (int d = 32; d >= 1; d >>= 1) { o |= __shfl_xor(o, d); a &= __shfl_xor(a, d); }
        if (lane == 0) {
            if (o & ~__atomic_load_n(col_or + w, __ATOMIC_RELAXED)) atomicOr(col_or + w, o);
            if (~a & __atomic_load_n(col_and + w, __ATOMIC_RELAXED)) atomicAnd(col_and + w, a);
        }
    }
}

__global__ __launch_bounds__(256) void k_namesort_identity(uint64_t n, uint32_t *idx)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) idx[i] = (uint32_t)i;
}

// one column in the current order: the 32-bit keys of the next pass
__global__ __launch_bounds__(256) void k_namesort_column(const uint32_t *column, const uint32_t *idx, uint64_t n, uint32_t *key)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) key[i] = column[idx[i]];
}

namespace {

template <class T> void need(DevBuf<T> &b, size_t n) { if (b.n < n) b.alloc(n); }

struct Buffers {                                    // grow-only, kept between calls (never destroyed: a writer may run during exit)
    int device = -1;
    DevBuf<uint8_t> src, out; DevBuf<uint64_t> off, key_a, key_b, slen, doff; DevBuf<uint32_t> len, idx_a, idx_b, col, col_bits; DevBuf<int32_t> ref, pos;   // col, col_bits: the name order's rows and their OR / AND
    PinBuf pin;
    void release() { src.release(); out.release(); off.release(); key_a.release(); key_b.release(); slen.release(); doff.release(); len.release(); idx_a.release(); idx_b.release(); ref.release(); pos.release(); col.release(); col_bits.release(); }
    void release_host() { if (pin.p) pin_cache_give(pin.p, pin.bytes); pin.p = nullptr; pin.bytes = 0; }
};
std::mutex g_mu;
Buffers &buffers() { static Buffers *b = new Buffers(); return *b; }
// One order's switch: the device it names (-1: off), the totals of its calls since it was last set, and what ties it to ps_bam.cpp --
// the environment variable that sets it when the library is loaded, where the hook is registered, the hook.  Two instances, never
// destroyed (a writer may run during exit).
template <class Stats> struct Switch {
    const char *env; void (*set_hook)(BamSortFn); BamSortFn hook;
    std::atomic<int> device{-1}; std::mutex mu; Stats total;
    Switch(const char *e, void (*set)(BamSortFn), BamSortFn h) : env(e), set_hook(set), hook(h) {}
};
bool device_hook(BamSortJob &job);
bool name_device_hook(BamSortJob &job);
Switch<BamSortStats> &by_coordinate() { static auto *s = new Switch<BamSortStats>("PS_BAM_SORT_GPU", &bam_sort_set_device_hook, &device_hook); return *s; }
Switch<BamNameSortStats> &by_name() { static auto *s = new Switch<BamNameSortStats>("PS_BAM_NAME_SORT_GPU", &bam_name_sort_set_device_hook, &name_device_hook); return *s; }

void copy_threads(void *dst, const void *src, size_t n)
{
    ranges(n, n >= ((size_t)4 << 20) ? 8 : 1, [&](size_t a0, size_t a1) { std::memcpy((char *)dst + a0, (const char *)src + a0, a1 - a0); });
}

// the two halves of the staging, `piece` bytes each: half() waits until the copy that last used the half is over, sent() marks the one
// just enqueued
struct Stager {
    uint8_t *base; size_t piece; hipStream_t s; hipEvent_t ev[2] = {nullptr, nullptr}; bool used[2] = {false, false}; int cur = 0;
    Stager(uint8_t *pin, size_t piece_bytes, hipStream_t stream) : base(pin), piece(piece_bytes), s(stream)
    {
        PS_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
        if (hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) != hipSuccess) { (void)hipEventDestroy(ev[0]); throw Error("hipEventCreate failed"); }
    }
    Stager(const Stager &) = delete;
    ~Stager() { (void)hipStreamSynchronize(s); (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]); }
    uint8_t *half() { if (used[cur]) { PS_HIP(hipEventSynchronize(ev[cur])); used[cur] = false; } return base + (size_t)cur * piece; }
    void sent() { PS_HIP(hipEventRecord(ev[cur], s)); used[cur] = true; cur ^= 1; }
    void wait_all() { PS_HIP(hipStreamSynchronize(s)); used[0] = used[1] = false; }
};

uint64_t max_device_bytes()
{
    long long mb = 32768;
    if (const char *e = std::getenv("PS_BAM_SORT_MAX_MB")) if (e[0]) mb = std::atoll(e);
    return mb < 0 ? 0 : (uint64_t)mb << 20;
}

// what the name order counts beside the common fields
void count_own(BamSortStats &, const BamSortStats &) {}
void count_own(BamNameSortStats &t, const BamNameSortStats &x) { t.n_passes += x.n_passes; if (x.n_calls_device) t.key_words = x.key_words; t.ms_keys += x.ms_keys; }
template <class Stats> void count(Switch<Stats> &sw, const Stats &x)
{
    std::lock_guard<std::mutex> l(sw.mu); Stats &t = sw.total;
    t.n_records += x.n_records; t.bytes += x.bytes; t.n_calls_device += x.n_calls_device; t.n_calls_host += x.n_calls_host; t.n_resident += x.n_resident;
    t.ms_upload += x.ms_upload; t.ms_sort += x.ms_sort; t.ms_gather += x.ms_gather; t.ms_download += x.ms_download;
    count_own(t, x);
}
void count(const BamSortStats &x) { count(by_coordinate(), x); }
void count(const BamNameSortStats &x) { count(by_name(), x); }

// The sorted stream of one call that stayed on the device, between the sort and the compression of its blocks (ps_bam.h: the device
// case of a BamBody): the buffer is taken out of the grow-only set for that time (another thread's sort gets its own) and goes back
// when the stream is destroyed -- if it is larger than what the set holds by then; otherwise it is freed.  One at a time: a second
// call that finds the slot taken brings its stream down as usual.  run_route claims the slot before its first device call, so an
// error on the way frees it with the empty stream.
std::atomic<bool> g_resident_taken{false};
struct ResidentStream : DeviceStream {
    DevBuf<uint8_t> out; uint64_t bytes = 0; int device = -1;
    static std::unique_ptr<ResidentStream> claim() { bool taken = false; return std::unique_ptr<ResidentStream>(g_resident_taken.compare_exchange_strong(taken, true) ? new ResidentStream() : nullptr); }
    ~ResidentStream() override
    {
        if (out.p) {
            std::lock_guard<std::mutex> lock(g_mu);
            Buffers &b = buffers();
            QuietDeviceScope scope(device);
            if (scope.ok) { if (b.device == device && b.out.n < out.n) b.out = std::move(out); else out.release(); }
        }
        g_resident_taken = false;
    }
    void blocks(std::string *comp) override { bgzf_device_compress_resident(out.p, bytes, device, comp, nullptr); }
};

bool device_hook(BamSortJob &job) { return bam_sort_device_run(job, by_coordinate().device, nullptr); }
bool name_device_hook(BamSortJob &job) { return bam_name_sort_device_run(job, by_name().device, nullptr); }

// PS_BAM_SORT_GPU=<device>, PS_BAM_NAME_SORT_GPU=<device>: read once, when the library is loaded; a device that is not there fails the first sorting call
template <class Stats> void read_env(Switch<Stats> &sw)
{
    const char *e = std::getenv(sw.env);
    if (e && e[0]) { const int d = std::atoi(e); if (d >= 0) { sw.device = d; sw.set_hook(sw.hook); } }
}
[[maybe_unused]] const bool g_env_read = [] { read_env(by_coordinate()); read_env(by_name()); return true; }();

// what no switch needs any more goes back (g_mu held): the name order's rows when its switch is off, every device and page-locked
// buffer when both are
void release_unused()
{
    Buffers &b = buffers();
    const bool coordinate_on = by_coordinate().device >= 0, name_on = by_name().device >= 0;
    if (b.device >= 0 && !name_on) { QuietDeviceScope scope(b.device); if (scope.ok) { if (coordinate_on) { b.col.release(); b.col_bits.release(); } else b.release(); } }
    if (!coordinate_on && !name_on) { b.device = -1; b.release_host(); }
}

template <class Stats> void set_device(Switch<Stats> &sw, int device)
{
    if (device >= 0) check_device("ps_bam_sort", device);
    { std::lock_guard<std::mutex> l(sw.mu); sw.total = Stats(); }
    if (device < 0) {                               // switched off: the buffers go back too (a later ps_bam_sort_records takes its own again)
        sw.set_hook(nullptr); sw.device = -1;
        std::lock_guard<std::mutex> lock(g_mu);
        release_unused();
        return;
    }
    sw.device = device;
    sw.set_hook(sw.hook);
}

template <class Stats> void info(Switch<Stats> &sw, Stats &out)
{
    std::lock_guard<std::mutex> l(sw.mu);
    out = sw.total; out.on_device = sw.device >= 0;
}

// One call of either route.  The stages are the same for both orders: the records checked against their buffers and the memory bound
// (all before the first device call), upload, the order, destinations and gather, download, the resident hand-over.  An Order says
// what differs: a look at the records on the host (false: the call is the host's), the device memory of its own, the two 32-bit
// columns that go up with every record, and the sort, which leaves the permutation on the device and its times in st.
template <class Order> bool run_route(BamSortJob &job, int device, Order &order)
{
    auto &st = order.st;
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
    if (n >= ((uint64_t)1 << 32) || !order.look(job) || src_bytes + total + 64 * (uint64_t)n + ((uint64_t)32 << 20) + order.device_bytes(n) > max_device_bytes()) {
        st.n_calls_host = 1; count(st);
        return false;
    }
    st.on_device = 1; st.n_calls_device = 1; st.n_records = n; st.bytes = total;
    job.body->device.reset();
    std::unique_ptr<ResidentStream> stay;
    if (n && job.may_stay && bgzf_device_current() == device) stay = ResidentStream::claim();
    job.perm->assign(n, 0); job.body->host.assign(stay ? 0 : (size_t)total, '\0');
    if (n == 0) { count(st); return true; }

    std::lock_guard<std::mutex> lock(g_mu);
    check_device("ps_bam_sort", device);
    DeviceScope scope(device);
    Buffers &b = buffers();
    if (b.device != device) { b.release(); b.device = device; }
    need(b.src, (size_t)((src_bytes + 3) & ~(uint64_t)3) + 16); need(b.out, (size_t)total + 16);
    need(b.off, n); need(b.len, n); need(b.ref, n); need(b.pos, n);
    need(b.key_a, n); need(b.key_b, n); need(b.idx_a, n); need(b.idx_b, n); need(b.slen, n + 1); need(b.doff, n + 1);
    order.need_buffers(b, n);
    const size_t PIECE = bamsort_piece_bytes(std::getenv("PS_BAM_SORT_PIECE"));    // one half of the page-locked staging (64 MiB; the knob is for tests)
    uint8_t *pin = (uint8_t *)b.pin.get(2 * PIECE);
    StreamGuard sg;
    Stager stg(pin, PIECE, sg.s);

    // ---- upload: the parts back to back, then the four columns (offset, length and the order's two), piece by piece
    HostClock::time_point t0 = HostClock::now();
    {
        BsCursor cur; uint64_t at = 0;
        while (at < src_bytes) {
            uint8_t *h = stg.half();
            size_t fill = 0;
            while (fill < PIECE && cur.part < job.n_parts) {
                const BsCut c = bamsort_next_cut(cur, job.parts[cur.part].n, PIECE - fill);
                if (c.take) copy_threads(h + fill, job.parts[c.part].p + c.in_part, c.take);
                fill += c.take;
            }
            PS_HIP(hipMemcpyAsync(b.src.p + at, h, fill, hipMemcpyHostToDevice, sg.s));
            stg.sent();
            at += fill;
        }
    }
    uint64_t any = 0;
    {
        const size_t per = bamsort_columns_per_piece(PIECE);           // off 8, len 4, ref 4, pos 4 per record
        const BsColumnsAt col = bamsort_columns_at(per);
        for (size_t i0 = 0; i0 < n; i0 += per) {
            const size_t m = std::min(per, n - i0);
            uint8_t *h = stg.half();
            uint64_t *h_off = (uint64_t *)(h + col.off); uint32_t *h_len = (uint32_t *)(h + col.len); int32_t *h_ref = (int32_t *)(h + col.ref), *h_pos = (int32_t *)(h + col.pos);
            std::atomic<uint64_t> any_piece{0};
            ranges(m, m >= 65536 ? 8 : 1, [&](size_t a0, size_t a1) {
                uint64_t o = 0;
                for (size_t j = a0; j < a1; ++j) {
                    const BamRec &r = job.recs[i0 + j];
                    h_off[j] = base[(size_t)r.part] + r.off; h_len[j] = (uint32_t)r.len;
                    o |= order.columns(i0 + j, r, h_ref[j], h_pos[j]);
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

    // ---- the order
    const uint32_t *perm = order.sort(b, sg.s, n, any, t0);
    t0 = HostClock::now();

    // ---- destinations, then the bytes
    hipLaunchKernelGGL(k_bamsort_lens, dim3(blocks_for(n + 1)), dim3(256), 0, sg.s, perm, b.len.p, (uint64_t)n, b.slen.p);
    PS_HIP(hipGetLastError());
    cub_call(sg.s, [&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, b.slen.p, b.doff.p, n + 1, sg.s); });
    uint64_t d_total = 0;
    PS_HIP(hipMemcpyAsync(&d_total, b.doff.p + n, sizeof d_total, hipMemcpyDeviceToHost, sg.s));
    PS_HIP(hipStreamSynchronize(sg.s));
    if (d_total != total) throw Error("ps_bam_sort: the device's offsets do not end at the records' size");
    BsArgs a{b.src.p, b.off.p, b.len.p, perm, b.doff.p, (uint64_t)n, b.out.p};
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
        down((const uint8_t *)perm, (char *)job.perm->data(), n * sizeof(uint32_t));
        if (!stay) down(b.out.p, &job.body->host[0], (size_t)total);
        stg.wait_all();
        if (prev.h) copy_threads(prev.dst, prev.h, prev.bytes);
    }
    st.ms_download = ms_since(t0);
    if (stay) {                                     // the stream's buffer leaves the set until the body is destroyed
        stay->out = std::move(b.out); stay->bytes = total; stay->device = device;
        job.body->device = std::move(stay);
        st.n_resident = 1;
    }
    count(st);
    static const bool verbose = std::getenv("PS_VERBOSE") != nullptr;
    if (verbose) order.report(n, total, device, st.n_resident ? " (the permutation alone: the stream stays for the compressor)" : "");
    return true;
}

// the coordinate order: ref and pos go up, ps_bamsort.h's 64-bit key is sorted over the bits that any key has set
struct CoordinateOrder {
    BamSortStats st; int end_bit = 0;
    bool look(const BamSortJob &) { return true; }
    uint64_t device_bytes(size_t) { return 0; }
    void need_buffers(Buffers &, size_t) {}
    uint64_t columns(size_t, const BamRec &r, int32_t &ref, int32_t &pos) { ref = r.ref; pos = r.pos; return bamsort_key(r.ref, r.pos); }
    const uint32_t *sort(Buffers &b, hipStream_t s, size_t n, uint64_t any, HostClock::time_point t0)
    {
        // keys, the sort over the bits that any key has set (all placed: 32 + the bits of the largest reference id)
        end_bit = bamsort_end_bit(any);
        hipLaunchKernelGGL(k_bamsort_keys, dim3(blocks_for(n)), dim3(256), 0, s, b.ref.p, b.pos.p, (uint64_t)n, b.key_a.p, b.idx_a.p);
        PS_HIP(hipGetLastError());
        cub_call(s, [&](void *tmp, size_t &bytes) { return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, b.key_a.p, b.key_b.p, b.idx_a.p, b.idx_b.p, n, 0, end_bit, s); });
        st.ms_sort = ms_since(t0);
        return b.idx_b.p;
    }
    void report(size_t n, uint64_t total, int device, const char *stayed)
    {
        std::fprintf(stderr, "[parasuite-hip] bam sort: %zu records, %.1f MB on device %d: upload %.1f ms, keys + sort over %d bits %.1f ms, offsets + gather %.1f ms, download %.1f ms%s\n",
                     n, total / 1e6, device, st.ms_upload, end_bit, st.ms_sort, st.ms_gather, st.ms_download, stayed);
    }
};

// The name order.  look(): every record's name must end inside the record (the length byte at 12 counts the NUL; the name is what
// strnum_cmp reads: up to the first NUL) -- the lengths, the longest one and with it the row's width, before any device call.  The
// two columns are the name's length and the pair bits of the flag.
struct NameOrder {
    BamNameSortStats st; std::vector<uint8_t> name_len; uint32_t longest = 0, W = 0;
    bool look(const BamSortJob &job)
    {
        const HostClock::time_point t0 = HostClock::now();
        const size_t n = job.n_recs;
        name_len.assign(n, 0);
        std::atomic<uint32_t> most{0}; std::atomic<bool> ok{true};
        ranges(n, n >= 65536 ? 8 : 1, [&](size_t a0, size_t a1) {
            uint32_t m = 0;
            for (size_t i = a0; i < a1; ++i) {
                const BamRec &r = job.recs[i];
                const uint8_t *p = (const uint8_t *)job.parts[r.part].p + r.off;
                if (!name_ends_inside(p, r.len)) { ok = false; return; }
                const uint32_t l = (uint32_t)strnlen((const char *)p + 36, p[12] - 1u);
                name_len[i] = (uint8_t)l; m = std::max(m, l);
            }
            uint32_t seen = most.load();
            while (seen < m && !most.compare_exchange_weak(seen, m)) {}
        });
        longest = most; W = namesort_words(longest);
        st.ms_keys = ms_since(t0);
        return ok && longest <= NS_MAX_NAME;
    }
    uint64_t device_bytes(size_t n) { return 4 * (uint64_t)W * n + 8 * (uint64_t)W; }
    void need_buffers(Buffers &b, size_t n) { need(b.col, (size_t)W * n); need(b.col_bits, 2 * (size_t)W); }
    uint64_t columns(size_t i, const BamRec &r, int32_t &len, int32_t &pair) { len = name_len[i]; pair = (int32_t)namesort_pair(r.flag); return 0; }
    const uint32_t *sort(Buffers &b, hipStream_t s, size_t n, uint64_t, HostClock::time_point t0)
    {
        // rows, column-major, with the OR and the AND of every column; the identity
        uint32_t *d_or = b.col_bits.p, *d_and = b.col_bits.p + W;
        PS_HIP(hipMemsetAsync(d_or, 0, 4 * (size_t)W, s)); PS_HIP(hipMemsetAsync(d_and, 0xff, 4 * (size_t)W, s));
        hipLaunchKernelGGL(k_namesort_rows, dim3((unsigned)((n + NS_NL - 1) / NS_NL)), dim3(NS_NL), 0, s, (const uint8_t *)b.src.p, (const uint64_t *)b.off.p, (const int32_t *)b.ref.p, (const int32_t *)b.pos.p, (uint64_t)n, W, b.col.p, d_or, d_and);
        PS_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_namesort_identity, dim3(blocks_for(n)), dim3(256), 0, s, (uint64_t)n, b.idx_a.p);
        PS_HIP(hipGetLastError());
        std::vector<uint32_t> bits(2 * (size_t)W);
        PS_HIP(hipMemcpyAsync(bits.data(), b.col_bits.p, 8 * (size_t)W, hipMemcpyDeviceToHost, s));
        PS_HIP(hipStreamSynchronize(s));
        st.ms_keys += ms_since(t0); t0 = HostClock::now();
        // least significant column first; a stable sort per column whose words differ, over the bits in which they do
        uint32_t *key_in = (uint32_t *)b.key_a.p, *key_out = (uint32_t *)b.key_b.p, *idx_in = b.idx_a.p, *idx_out = b.idx_b.p;
        DevBuf<uint8_t> tmp;
        for (uint32_t w = W; w-- > 0;) {
            const uint32_t diff = bits[w] ^ bits[W + w];
            if (!diff) continue;
            hipLaunchKernelGGL(k_namesort_column, dim3(blocks_for(n)), dim3(256), 0, s, (const uint32_t *)(b.col.p + (size_t)w * n), (const uint32_t *)idx_in, (uint64_t)n, key_in);
            PS_HIP(hipGetLastError());
            const int b0 = namesort_begin_bit(diff), b1 = namesort_end_bit(diff);
            size_t bytes = 0;
            PS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, key_in, key_out, idx_in, idx_out, n, b0, b1, s));
            if (tmp.n < std::max<size_t>(bytes, 1)) tmp.alloc(std::max<size_t>(bytes, 1));
            PS_HIP(hipcub::DeviceRadixSort::SortPairs((void *)tmp.p, bytes, key_in, key_out, idx_in, idx_out, n, b0, b1, s));
            std::swap(idx_in, idx_out);
            ++st.n_passes;
        }
        PS_HIP(hipStreamSynchronize(s));
        st.key_words = W;
        st.ms_sort = ms_since(t0);
        return idx_in;
    }
    void report(size_t n, uint64_t total, int device, const char *stayed)
    {
        std::fprintf(stderr, "[parasuite-hip] bam name sort: %zu records, %.1f MB on device %d: upload %.1f ms, rows of %u words %.1f ms, %llu column sorts %.1f ms, offsets + gather %.1f ms, download %.1f ms%s\n",
                     n, total / 1e6, device, st.ms_upload, W, st.ms_keys, (unsigned long long)st.n_passes, st.ms_sort, st.ms_gather, st.ms_download, stayed);
    }
};


}  // namespace

void bam_sort_set_device(int device) { set_device(by_coordinate(), device); }
void bam_sort_info(BamSortStats &out) { info(by_coordinate(), out); }
void bam_name_sort_set_device(int device) { set_device(by_name(), device); }
void bam_name_sort_info(BamNameSortStats &out) { info(by_name(), out); }

template <class Order, class Stats> static bool run_order(BamSortJob &job, int device, Stats *stats)
{
    Order order;
    const bool done = run_route(job, device, order);
    if (stats) *stats = order.st;
    return done;
}
bool bam_sort_device_run(BamSortJob &job, int device, BamSortStats *stats) { return run_order<CoordinateOrder>(job, device, stats); }
bool bam_name_sort_device_run(BamSortJob &job, int device, BamNameSortStats *stats) { return run_order<NameOrder>(job, device, stats); }

}  // namespace ps
