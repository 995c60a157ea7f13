// ps_par.h -- contiguous ranges of a host loop on a few threads.
#pragma once
#include <algorithm>
#include <exception>
#include <thread>
#include <vector>

namespace ps {

// host loops over millions of reads: contiguous ranges on a few threads; f(begin, end, thread)
template <class F> void par_for(size_t n, int threads, F f)
{
    size_t nt = (size_t)std::max(1, threads);
    if (nt > n / 8192 + 1) nt = n / 8192 + 1;
    if (nt <= 1) { if (n) f((size_t)0, n, 0); return; }
    std::vector<std::thread> th;
    std::vector<std::exception_ptr> err(nt);
    const size_t per = (n + nt - 1) / nt;
    for (size_t t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
            const size_t a0 = t * per, b0 = std::min(n, a0 + per);
            try { if (a0 < b0) f(a0, b0, (int)t); } catch (...) { err[t] = std::current_exception(); }
        });
    for (auto &x : th) x.join();
    for (auto &e : err) if (e) std::rethrow_exception(e);
}
inline int par_threads(size_t n, int threads) { size_t nt = (size_t)std::max(1, threads); if (nt > n / 8192 + 1) nt = n / 8192 + 1; return (int)std::max<size_t>(1, nt); }

}  // namespace ps
