// ps_bgzf.hip -- the BGZF blocks of a BAM compressed on the device: what ps_bam.cpp's batch function hands over when the switch is
// on (ps_bgzf_device, PS_BGZF_GPU), and ps_bgzf_compress.  One workgroup of 64 lanes per block runs ps_deflate.h's encoder; the host
// side stages the spans back to back in page-locked memory, uploads them with their offsets, launches once per round, downloads
// the sizes and CRCs, packs the images on the device, downloads them and puts the 18-byte member header and the 8-byte trailer around each.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#define PS_DF_DEVICE
#include "ps_deflate.h"
#include "ps_bgzf.h"
#include "ps_dev.h"
#include "ps_pipeline.h"

namespace ps {

static_assert(sizeof(DfShared) <= 48 * 1024, "k_bgzf: static LDS");
static_assert((size_t)DF_BLOCK == kBgzfBlock, "the encoder's block is the writers' cut");
static_assert(DF_OUT_STRIDE % 16 == 0 && DF_OUT_STRIDE >= DF_BLOCK + 8, "k_bgzf: room for n + 5 bytes in whole words");

// block k of the round: in[offs[k], offs[k + 1]) -> out + k * DF_OUT_STRIDE, res[k]; tok: one word per input byte of the round
__global__ __launch_bounds__(DF_NL) void k_bgzf(const uint8_t *in, const uint64_t *offs, uint32_t n_blocks, uint8_t *out, uint32_t *tok, DfResult *res, uint32_t allow)
{
    __shared__ DfShared sh;
    const uint32_t k = blockIdx.x;
    if (k >= n_blocks) return;
    const uint64_t a = offs[k];
    const uint32_t n = (uint32_t)(offs[k + 1] - a);
    if (n > DF_BLOCK) return;                       // the host never asks for it; res[k] stays zero and the host fails the call
    df_block(sh, in + a, n, (uint32_t *)(out + (size_t)k * DF_OUT_STRIDE), tok + a, allow, res + k);
}

// the images of a round moved together: image k (res[k].bytes bytes, copied in whole words) -> packed + at[k]; the host sums the
// sizes, each rounded up to a word, so that only what was produced crosses to the host
__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t *out, const DfResult *res, const uint64_t *at, uint32_t n_blocks, uint8_t *packed)
{
    const uint32_t k = blockIdx.x;
    if (k >= n_blocks) return;
    const uint32_t words = (res[k].bytes + 3) / 4;
    if (words > DF_OUT_STRIDE / 4) return;          // no image is that long (n + 5 bytes at most): the host has refused the round by then
    const uint32_t *src = (const uint32_t *)(out + (size_t)k * DF_OUT_STRIDE);
    uint32_t *dst = (uint32_t *)(packed + at[k]);
    for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) dst[w] = src[w];
}

namespace {

struct Buffers {                                    // grow-only, kept between calls (never destroyed: a writer may run during exit)
    int device = -1;
    DevBuf<uint8_t> in, out, packed; DevBuf<uint32_t> tok; DevBuf<uint64_t> offs; DevBuf<DfResult> res;
    PinBuf pin;
    void release() { in.release(); out.release(); packed.release(); tok.release(); offs.release(); res.release(); }
    void release_host() { if (pin.p) pin_cache_give(pin.p, pin.bytes); pin.p = nullptr; pin.bytes = 0; }
};
std::mutex g_mu;
Buffers &buffers() { static Buffers *b = new Buffers(); return *b; }
std::atomic<int> g_device{-1};

uint32_t allowed_encodings()
{
    const char *e = std::getenv("PS_BGZF_BTYPE");
    if (!e || !e[0]) return DF_ALL;
    const std::string v = e;
    if (v == "stored") return DF_STORED;
    if (v == "fixed") return DF_FIXED;
    if (v == "dynamic") return DF_DYNAMIC;
    throw Error("PS_BGZF_BTYPE is stored, fixed or dynamic");
}

size_t blocks_per_round()
{
    size_t piece = (size_t)64 << 20;
    if (const char *e = std::getenv("PS_BGZF_PIECE")) { const long long v = std::atoll(e); if (v > 0) piece = (size_t)v; }
    return std::max<size_t>(1, std::min<size_t>(piece / DF_BLOCK, 16384));
}

void device_batch(const BgzfSpan *spans, size_t n_spans, std::string *comp) { bgzf_device_compress(spans, n_spans, g_device, comp, nullptr); }

// PS_BGZF_GPU=<device>: read once, when the library is loaded; a device that is not there fails the first writing call
[[maybe_unused]] const bool g_env_read = [] {
    const char *e = std::getenv("PS_BGZF_GPU");
    if (e && e[0]) { const int d = std::atoi(e); if (d >= 0) { g_device = d; bgzf_set_device_compressor(&device_batch); } }
    return true;
}();

}  // namespace

void bgzf_set_device(int device)
{
    if (device < 0) {                               // switched off: the buffers go back too (a later ps_bgzf_compress takes its own again)
        bgzf_set_device_compressor(nullptr); g_device = -1;
        std::lock_guard<std::mutex> lock(g_mu);
        Buffers &b = buffers();
        if (b.device >= 0) { QuietDeviceScope scope(b.device); if (scope.ok) b.release(); b.device = -1; }
        b.release_host();
        return;
    }
    check_device("ps_bgzf", device);
    g_device = device;
    bgzf_set_device_compressor(&device_batch);
}

int bgzf_device_current() { return g_device; }

// spans on the host (staged and uploaded round by round), or -- spans null -- d_stream[0, n_bytes) on `device` cut at 0xff00 bytes:
// a round's kernel then reads the stream where it lies, and neither the staging copy nor the upload happens
static void compress_rounds(const BgzfSpan *spans, size_t n_spans, const uint8_t *d_stream, uint64_t n_bytes, int device, std::string *comp, BgzfStats *stats)
{
    BgzfStats st;
    auto n_of = [&](size_t k) { return spans ? spans[k].n : (size_t)std::min<uint64_t>((uint64_t)DF_BLOCK, n_bytes - (uint64_t)k * DF_BLOCK); };
    for (size_t k = 0; spans && k < n_spans; ++k) if (spans[k].n > (size_t)DF_BLOCK) throw Error("ps_bgzf: a span of more than 0xff00 bytes");
    if (n_spans) {
        const uint32_t allow = allowed_encodings();
        const size_t per_round = std::min(blocks_per_round(), n_spans);
        const bool verbose = std::getenv("PS_VERBOSE") != nullptr;
        const HostClock::time_point t_ask = HostClock::now();
        std::lock_guard<std::mutex> lock(g_mu);
        const double ms_lock = ms_since(t_ask);
        const HostClock::time_point t_begin = HostClock::now();
        double ms_device = 0;                       // first upload to last byte down, summed over the rounds
        check_device("ps_bgzf", device);
        DeviceScope scope(device);
        Buffers &b = buffers();
        if (b.device != device) { b.release(); b.device = device; }
        const size_t in_cap = per_round * (size_t)DF_BLOCK, out_cap = per_round * (size_t)DF_OUT_STRIDE;
        if (spans && b.in.n < in_cap) b.in.alloc(in_cap);
        if (b.tok.n < in_cap) b.tok.alloc(in_cap);
        if (b.out.n < out_cap) { b.out.alloc(out_cap); b.packed.alloc(out_cap); }
        if (b.offs.n < per_round + 1) { b.offs.alloc(per_round + 1); b.res.alloc(per_round); }
        // page-locked staging: input | offsets | results | images
        const size_t at_offs = (in_cap + 15) & ~(size_t)15, at_res = at_offs + (per_round + 1) * sizeof(uint64_t),
                     at_out = (at_res + per_round * sizeof(DfResult) + 15) & ~(size_t)15;
        uint8_t *pin = (uint8_t *)b.pin.get(at_out + out_cap);
        uint64_t *h_offs = (uint64_t *)(pin + at_offs); DfResult *h_res = (DfResult *)(pin + at_res); uint8_t *h_out = pin + at_out;
        StreamGuard sg;
        EventPair ev;
        for (size_t r0 = 0; r0 < n_spans; r0 += per_round) {
            const size_t nb = std::min(per_round, n_spans - r0);
            h_offs[0] = 0;
            for (size_t k = 0; k < nb; ++k) h_offs[k + 1] = h_offs[k] + n_of(r0 + k);
            const size_t bytes = (size_t)h_offs[nb];
            if (spans) ranges(nb, bytes >= ((size_t)4 << 20) ? 8 : 1, [&](size_t k0, size_t k1) { for (size_t k = k0; k < k1; ++k) if (spans[r0 + k].n) std::memcpy(pin + h_offs[k], spans[r0 + k].p, spans[r0 + k].n); });
            const HostClock::time_point t_dev = HostClock::now();
            if (spans && bytes) b.in.upload(pin, bytes, sg.s);
            const uint8_t *d_in = spans ? b.in.p : d_stream + (uint64_t)r0 * DF_BLOCK;      // the round's first byte: the offsets count from it
            b.offs.upload(h_offs, nb + 1, sg.s);
            PS_HIP(hipMemsetAsync(b.res.p, 0, nb * sizeof(DfResult), sg.s));
            ev.start(sg.s);
            hipLaunchKernelGGL(k_bgzf, dim3((unsigned)nb), dim3(DF_NL), 0, sg.s, d_in, b.offs.p, (uint32_t)nb, b.out.p, b.tok.p, b.res.p, allow);
            PS_HIP(hipGetLastError());
            ev.stop(sg.s);
            b.res.download(h_res, nb, sg.s);
            PS_HIP(hipStreamSynchronize(sg.s));
            st.kernel_ms += ev.ms();
            for (size_t k = 0; k < nb; ++k)
                if (h_res[k].bytes == 0 || h_res[k].bytes > n_of(r0 + k) + 5 || h_res[k].btype > 2) throw Error("ps_bgzf: the device returned no valid block");
            // the sizes are known now: the images are packed on the device (each at a word boundary) and only they come down
            h_offs[0] = 0;
            for (size_t k = 0; k < nb; ++k) h_offs[k + 1] = h_offs[k] + (((uint64_t)h_res[k].bytes + 3) & ~(uint64_t)3);
            const size_t packed_bytes = (size_t)h_offs[nb];             // <= nb * DF_OUT_STRIDE: every image is at most n + 5 <= DF_OUT_STRIDE - 8 bytes
            b.offs.upload(h_offs, nb + 1, sg.s);
            ev.start(sg.s);
            hipLaunchKernelGGL(k_bgzf_pack, dim3((unsigned)nb), dim3(256), 0, sg.s, b.out.p, b.res.p, b.offs.p, (uint32_t)nb, b.packed.p);
            PS_HIP(hipGetLastError());
            ev.stop(sg.s);
            b.packed.download(h_out, packed_bytes, sg.s);
            PS_HIP(hipStreamSynchronize(sg.s));
            st.kernel_ms += ev.ms();
            ms_device += ms_since(t_dev);
            ranges(nb, bytes >= ((size_t)4 << 20) ? 8 : 1, [&](size_t k0, size_t k1) {
                for (size_t k = k0; k < k1; ++k) {
                    const DfResult &r = h_res[k];
                    comp[r0 + k].clear();
                    bgzf_member(h_out + h_offs[k], r.bytes, r.crc, (uint32_t)n_of(r0 + k), comp[r0 + k]);
                }
            });
            for (size_t k = 0; k < nb; ++k) {
                const DfResult &r = h_res[k];
                ++st.n_blocks; st.n_stored += r.btype == 0; st.n_fixed += r.btype == 1; st.n_dynamic += r.btype == 2;
                st.in_bytes += n_of(r0 + k); st.out_bytes += 18 + r.bytes + 8;
            }
        }
        if (verbose)
            std::fprintf(stderr, "[parasuite-hip] bgzf: %u blocks%s, %.1f MB -> %.1f MB on device %d in %.1f ms: waited %.1f ms for the compressor, device part %.1f ms (kernels %.1f ms), the rest staging and assembly\n",
                         st.n_blocks, spans ? "" : " of a stream that lay on the device", st.in_bytes / 1e6, st.out_bytes / 1e6, device, ms_since(t_begin) + ms_lock, ms_lock, ms_device, st.kernel_ms);
    }
    if (stats) *stats = st;
}

void bgzf_device_compress(const BgzfSpan *spans, size_t n_spans, int device, std::string *comp, BgzfStats *stats)
{
    static const BgzfSpan none{nullptr, 0};
    compress_rounds(spans ? spans : &none, n_spans, nullptr, 0, device, comp, stats);
}

void bgzf_device_compress_resident(const uint8_t *d_stream, uint64_t n_bytes, int device, std::string *comp, BgzfStats *stats)
{
    compress_rounds(nullptr, (size_t)((n_bytes + DF_BLOCK - 1) / DF_BLOCK), d_stream, n_bytes, device, comp, stats);
}

}  // namespace ps
