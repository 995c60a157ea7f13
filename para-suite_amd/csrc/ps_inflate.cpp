// ps_inflate.cpp -- the byte source of the text inputs: plain, gzip or BGZF (ps_inflate.h; host only, zlib).
#include <zlib.h>
#include <algorithm>
#include <cerrno>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <unistd.h>
#include <sys/stat.h>
#include "ps_inflate.h"
#include "ps_map_plan.h"

namespace ps {

namespace {

// `want` bytes at file offset `at` into dst, by a few threads side by side when the file is a regular one (one thread copies ~3 GB/s out
// of the page cache); returns the bytes read (fewer than wanted: the input ends there)
size_t read_at(const std::string &path, int fd, bool regular, off_t at, char *dst, size_t want, int threads)
{
    auto one = [&](size_t lo, size_t hi) -> size_t {
        size_t have = lo;
        while (have < hi) {
            const ssize_t r = regular ? ::pread(fd, dst + have, hi - have, at + (off_t)have) : ::read(fd, dst + have, hi - have);
            if (r < 0) { if (errno == EINTR) continue; throw Error("read error on " + path); }
            if (r == 0) break;
            have += (size_t)r;
        }
        return have - lo;
    };
    const int nt = regular ? (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(threads, 8), want >> 22)) : 1;      // >= 4 MB per thread
    if (nt == 1) return one(0, want);
    std::vector<size_t> got((size_t)nt, 0); std::vector<std::string> err((size_t)nt);
    auto part = [&](int t) { try { got[t] = one(want * (size_t)t / nt, want * (size_t)(t + 1) / nt); } catch (const std::exception &e) { err[t] = e.what(); } };
    { std::vector<std::thread> th; for (int t = 1; t < nt; ++t) th.emplace_back(part, t); part(0); for (auto &x : th) x.join(); }
    size_t total = 0;
    for (int t = 0; t < nt; ++t) {
        if (!err[t].empty()) throw Error(err[t]);
        total += got[t];
        if (got[t] < want * (size_t)(t + 1) / nt - want * (size_t)t / nt) break;       // the input ended inside this part: what lies behind is not there
    }
    return total;
}

struct Win { std::unique_ptr<char[]> p; size_t n = 0; };     // a window of text on its way from the inflater (not zero-filled)

}  // namespace

struct ByteSource::Impl {
    enum Kind { PLAIN, GZ_UNSEEN, GZIP, BGZF };
    std::string path; int fd = -1; bool regular = false; uint64_t fsize = 0; Kind kind = PLAIN; size_t window = 0;
    // plain: where the next read starts; the two bytes that told the kind, when they could not be put back (a FIFO)
    off_t file_at = 0; unsigned char pre[2] = {0, 0}; size_t n_pre = 0, pre_at = 0;
    // compressed: raw[r0, r1) is read and not yet decoded; raw[r0] lies at byte raw_off of the input
    std::vector<unsigned char> raw; size_t r0 = 0, r1 = 0; uint64_t raw_off = 0; bool raw_eof = false;
    uint64_t n_members = 0;
    // gzip: the inflater thread, its hand-over, the window being read out
    std::thread th; Chan<Win> chan; std::string err; bool ended = false;
    Win cur; size_t cur_at = 0;
    // BGZF: the block that did not fit into what was asked for
    std::vector<char> spill; size_t spill_at = 0;

    ~Impl()
    {
        if (th.joinable()) { chan.abort(); th.join(); }
        if (fd >= 0) ::close(fd);
    }
    [[noreturn]] void fail(const char *what, uint64_t off) const { throw Error(path + ": " + what + " at compressed byte " + std::to_string(off)); }
    // at least n bytes in raw[r0, r1) unless the input ends first; returns how many there are
    size_t need(size_t n)
    {
        if (r1 - r0 >= n || raw_eof) return r1 - r0;
        if (r0 == r1) r0 = r1 = 0;
        if (r0 && raw.size() - r0 < n) { std::memmove(raw.data(), raw.data() + r0, r1 - r0); r1 -= r0; r0 = 0; }
        if (raw.size() < r0 + n) raw.resize(std::max(r0 + n + n / 4, (size_t)1 << 20));
        while (r1 - r0 < n) {
            const ssize_t r = ::read(fd, raw.data() + r1, raw.size() - r1);
            if (r < 0) { if (errno == EINTR) continue; throw Error("read error on " + path); }
            if (r == 0) { raw_eof = true; break; }
            r1 += (size_t)r;
        }
        return r1 - r0;
    }
    void skip(size_t k) { r0 += k; raw_off += k; }
    // the member header at raw[r0 + at ..): its length and BSIZE + 1 (0: no BC subfield).  The input must not end inside it.
    void header(size_t at, size_t &hl, size_t &bs)
    {
        const char *why = nullptr;
        for (size_t ask = 64;; ask *= 2) {
            const size_t av = need(at + ask) - at;
            const unsigned char *h = raw.data() + r0 + at;
            if (n_members && (h[0] != 31 || (av >= 2 && h[1] != 139))) fail("bytes behind a complete member that do not start another member", raw_off + at);
            const int rc = gz_member_header(h, av, hl, bs, why);
            if (rc > 0) return;
            if (rc < 0) fail(why, raw_off + at);
            if (av < ask) fail("the input ends inside a member header", raw_off + at + av);
        }
    }
    bool closed() { std::lock_guard<std::mutex> l(chan.m); return chan.closed; }

    size_t read_plain(char *dst, size_t want, int threads)
    {
        size_t got = 0;
        while (pre_at < n_pre && got < want) dst[got++] = (char)pre[pre_at++];
        const size_t more = got < want ? read_at(path, fd, regular, file_at, dst + got, want - got, threads) : 0;
        file_at += (off_t)more;
        return got + more;
    }

    // ---- gzip: members one after the other on one thread, windows handed over as they fill
    void inflate_members()
    {
        Win w; size_t fill = 0;
        auto out = [&]() { w.n = fill; chan.push(std::move(w)); w = Win(); fill = 0; return !closed(); };
        struct ZEnd { z_stream *z; ~ZEnd() { inflateEnd(z); } };
        for (;;) {
            if (need(1) == 0 && n_members) break;                      // the input ends behind a complete member
            if (need(1) == 0) fail("the input ends inside a member header", raw_off);
            size_t hl, bs;
            header(0, hl, bs);
            skip(hl);
            z_stream zs; std::memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, -15) != Z_OK) throw Error("inflateInit2 failed");
            ZEnd guard{&zs};
            uint32_t crc = (uint32_t)crc32(0L, Z_NULL, 0); uint64_t total = 0;
            for (;;) {
                const size_t av = need(1);
                if (av == 0) fail("the input ends inside a member's data", raw_off);
                if (!w.p) w.p.reset(new char[window]);
                const size_t in0 = std::min<size_t>(av, (size_t)1 << 30), out0 = std::min<size_t>(window - fill, (size_t)1 << 30);
                zs.next_in = raw.data() + r0; zs.avail_in = (uInt)in0;
                zs.next_out = (Bytef *)w.p.get() + fill; zs.avail_out = (uInt)out0;
                const int rc = inflate(&zs, Z_NO_FLUSH);
                const size_t used = in0 - zs.avail_in, made = out0 - zs.avail_out;
                if (made) crc = (uint32_t)crc32(crc, (const Bytef *)w.p.get() + fill, (uInt)made);
                fill += made; total += made;
                skip(used);
                if (fill == window && !out()) return;                  // nobody reads any more
                if (rc == Z_STREAM_END) break;
                if ((rc != Z_OK && rc != Z_BUF_ERROR) || (used == 0 && made == 0)) fail("invalid deflate data", raw_off);
            }
            if (need(8) < 8) fail("the input ends inside a member's trailer", raw_off + (r1 - r0));
            if (le32(raw.data() + r0) != crc) fail("CRC32 mismatch in the member that ends", raw_off + 8);
            if (le32(raw.data() + r0 + 4) != (uint32_t)total) fail("ISIZE mismatch in the member that ends", raw_off + 8);
            skip(8);
            ++n_members;
        }
        if (fill) out();
    }
    void start_inflater()
    {
        kind = GZIP;
        chan.cap = 2;
        th = std::thread([this]() {
            try { inflate_members(); } catch (const std::exception &e) { err = e.what(); if (err.empty()) err = "error"; }
            chan.close();                                              // what is queued in front of an error is still handed out, then the error
        });
    }
    size_t read_gzip(char *dst, size_t want)
    {
        size_t got = 0;
        while (got < want) {
            if (cur_at == cur.n) {
                if (ended) { if (!err.empty()) throw Error(err); break; }
                Win w;
                if (!chan.pop(w)) { ended = true; continue; }
                cur = std::move(w); cur_at = 0;
                continue;
            }
            const size_t take = std::min(want - got, cur.n - cur_at);
            std::memcpy(dst + got, cur.p.get() + cur_at, take);
            got += take; cur_at += take;
        }
        return got;
    }

    // ---- BGZF: the blocks that fill what is asked for are found by their BSIZE, placed by their ISIZE and inflated side by side
    size_t read_bgzf(char *dst, size_t want, int threads)
    {
        size_t got = 0;
        while (got < want) {
            if (spill_at < spill.size()) {
                const size_t take = std::min(want - got, spill.size() - spill_at);
                std::memcpy(dst + got, spill.data() + spill_at, take);
                got += take; spill_at += take;
                continue;
            }
            if (kind == GZIP) return got + read_gzip(dst + got, want - got);
            if (ended) break;
            struct B { size_t at, bsize, hl; uint32_t isize; size_t out; bool spill; };
            std::vector<B> bl; size_t tot = 0, out = 0; bool to_serial = false;
            for (;;) {
                if (need(tot + 1) == tot) { ended = true; break; }
                size_t hl, bs;
                header(tot, hl, bs);
                if (bs == 0) { to_serial = true; break; }              // a member without BC: the serial decoder takes the rest
                if (bs < hl + 8) fail("a BSIZE too small for a block", raw_off + tot);
                if (need(tot + bs) - tot < bs) fail("a BSIZE that reaches past the end of the input", raw_off + tot);
                const uint32_t isize = bgzf_isize(raw.data() + r0 + tot, bs);
                if (isize > kBgzfMaxOut) fail("a BGZF block with ISIZE above 64 KiB", raw_off + tot);
                const bool fits = isize <= want - got - out;
                bl.push_back(B{tot, bs, hl, isize, out, !fits});
                tot += bs;
                if (!fits) break;                                      // inflated with the others, read out by the next call
                out += isize;
            }
            const size_t nb = bl.size();
            if (nb) {
                const unsigned char *base = raw.data() + r0;
                spill.clear(); spill_at = 0;
                if (bl.back().spill) spill.resize(bl.back().isize);
                const int T = (int)std::min<size_t>((size_t)std::max(1, std::min(threads, 64)), (nb + 7) / 8);      // >= 8 blocks per thread
                std::vector<const char *> bad((size_t)T, nullptr); std::vector<size_t> bad_at((size_t)T, 0);
                auto part = [&](int t) {
                    for (size_t k = nb * (size_t)t / (size_t)T; k < nb * ((size_t)t + 1) / (size_t)T; ++k) {
                        const B &b = bl[k];
                        const char *e = bgzf_inflate_block(base + b.at, b.bsize, b.hl, b.spill ? spill.data() : dst + got + b.out, b.isize);
                        if (e) { bad[t] = e; bad_at[t] = b.at; return; }
                    }
                };
                { std::vector<std::thread> th2; for (int t = 1; t < T; ++t) th2.emplace_back(part, t); part(0); for (auto &x : th2) x.join(); }
                for (int t = 0; t < T; ++t) if (bad[t]) { spill.clear(); fail(bad[t], raw_off + bad_at[t]); }
                skip(tot); n_members += nb; got += out;
            }
            if (to_serial) start_inflater();
        }
        return got;
    }
};

ByteSource::ByteSource(const char *path, const char *open_error, size_t window) : p(nullptr)
{
    std::unique_ptr<Impl> q(new Impl());
    q->path = path; q->window = std::max(window, (size_t)64 << 10);
    q->fd = ::open(path, O_RDONLY);
    if (q->fd < 0) throw Error(std::string(open_error) + path);
    struct stat st;
    q->regular = ::fstat(q->fd, &st) == 0 && S_ISREG(st.st_mode);
    if (q->regular) q->fsize = (uint64_t)st.st_size;
    unsigned char mg[2] = {0, 0}; size_t n = 0;
    while (n < 2) {
        const ssize_t r = q->regular ? ::pread(q->fd, mg + n, 2 - n, (off_t)n) : ::read(q->fd, mg + n, 2 - n);
        if (r < 0) { if (errno == EINTR) continue; throw Error(std::string("read error on ") + path); }
        if (r == 0) break;
        n += (size_t)r;
    }
    if (n == 2 && mg[0] == 31 && mg[1] == 139) {
        q->kind = Impl::GZ_UNSEEN;
        if (!q->regular) { q->raw.resize((size_t)1 << 20); q->raw[0] = mg[0]; q->raw[1] = mg[1]; q->r1 = 2; }
    } else if (!q->regular) { q->pre[0] = mg[0]; q->pre[1] = mg[1]; q->n_pre = n; }
    p = q.release();
}
ByteSource::~ByteSource() { delete p; }
bool ByteSource::compressed() const { return p->kind != Impl::PLAIN; }
bool ByteSource::size_known() const { return p->kind == Impl::PLAIN && p->regular; }
uint64_t ByteSource::size() const { return p->fsize; }
size_t ByteSource::read(char *dst, size_t want, int threads)
{
    if (want == 0) return 0;
    if (p->kind == Impl::PLAIN) return p->read_plain(dst, want, threads);
    if (p->kind == Impl::GZ_UNSEEN) {
        // BGZF if the first member is well-formed and carries BC; everything else, a damaged header included, is the serial decoder's
        size_t hl = 0, bs = 0; const char *why = nullptr; int rc = 0;
        for (size_t ask = 64; rc == 0; ask *= 2) {
            const size_t av = p->need(ask);
            rc = gz_member_header(p->raw.data() + p->r0, av, hl, bs, why);
            if (av < ask) break;
        }
        if (rc > 0 && bs) p->kind = Impl::BGZF; else p->start_inflater();
    }
    return p->kind == Impl::BGZF ? p->read_bgzf(dst, want, threads) : p->read_gzip(dst, want);
}

bool is_gzip_file(const char *path)
{
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat st; unsigned char mg[2] = {0, 0};
    const bool gz = ::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && ::pread(fd, mg, 2, 0) == 2 && mg[0] == 31 && mg[1] == 139;
    ::close(fd);
    return gz;
}

}  // namespace ps
