// map_plan_check.cpp -- stand-alone driver of csrc/ps_map_plan.h for tests/test_map_plan_cpu.py (host compiler, sanitizers on).
//   map_plan_check devices (<ids or -> <gpus> <per_dev> <present> <max_lanes>)...   one line per case: "d,d,.. w,w,.."
//   map_plan_check pieces (<bytes> <workers> <bam> <chunk_mb> <hungry_mb> <first_mb>)...   one line per case: "chunk hungry first"
//   map_plan_check chan                                                             the hand-over queue; prints "chan ok"
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include "ps_map_plan.h"

using namespace ps;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static int chan_checks()
{
    {   // bounded by cap: pushes that have returned never lead the pops by more than cap
        Chan<int> c; c.cap = 2;
        std::atomic<int> pushed{0};
        std::thread producer([&] { for (int i = 0; i < 40; ++i) { c.push(int(i)); ++pushed; } c.close(); });
        int v = -1, popped = 0;
        while (c.pop(v)) {
            CHECK(v == popped);                                  // in order
            ++popped;
            CHECK(pushed.load() <= popped + (int)c.cap);
            { std::lock_guard<std::mutex> l(c.m); CHECK(c.q.size() <= c.cap); }
        }
        producer.join();
        CHECK(popped == 40);
    }
    {   // close(): what is queued is still handed out, then pop returns false; a push after it is dropped
        Chan<int> c; int v = 0;
        CHECK(!c.hungry());                                      // nobody waits
        c.push(7); c.push(8);
        CHECK(!c.hungry());                                      // no waiter, and the queue is not empty
        c.close();
        c.push(9);
        CHECK(c.pop(v) && v == 7); CHECK(c.pop(v) && v == 8); CHECK(!c.pop(v)); CHECK(!c.pop(v));
    }
    {   // abort(): drops the queue and releases a blocked push
        Chan<int> c; c.cap = 1; int v = 0;
        c.push(1);
        std::thread producer([&] { c.push(2); });               // the queue is full: blocks until the abort (or finds the channel closed)
        c.abort();
        producer.join();
        CHECK(!c.pop(v));
        { std::lock_guard<std::mutex> l(c.m); CHECK(c.q.empty()); }
    }
    {   // abort() releases a blocked pop; hungry() is true exactly while somebody waits at an empty queue
        Chan<int> c; std::atomic<int> got{-1};
        std::thread consumer([&] { int v = 0; got = c.pop(v) ? 1 : 0; });
        while (!c.hungry()) std::this_thread::yield();          // the consumer has arrived in pop()
        c.abort();
        consumer.join();
        CHECK(got.load() == 0);
        CHECK(!c.hungry());
    }
    {   // a waiting consumer is served by the next push, and is hungry no more
        Chan<int> c; std::atomic<int> got{-1};
        std::thread consumer([&] { int v = 0; if (c.pop(v)) got = v; });
        while (!c.hungry()) std::this_thread::yield();
        c.push(5);
        consumer.join();
        CHECK(got.load() == 5);
        CHECK(!c.hungry());
    }
    std::puts("chan ok");
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "chan") return chan_checks();
    if (mode == "devices" && (argc - 2) % 5 == 0) {
        for (int i = 2; i < argc; i += 5) {
            const DevicePlan d = plan_devices(std::strcmp(argv[i], "-") ? argv[i] : nullptr, std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]), std::atoi(argv[i + 4]));
            for (size_t k = 0; k < d.devs.size(); ++k) std::printf("%s%d", k ? "," : "", d.devs[k]);
            std::printf(" ");
            for (size_t k = 0; k < d.workers.size(); ++k) std::printf("%s%d", k ? "," : "", d.workers[k]);
            std::printf("\n");
        }
        return 0;
    }
    if (mode == "pieces" && (argc - 2) % 6 == 0) {
        for (int i = 2; i < argc; i += 6) {
            const PiecePlan p = plan_pieces((size_t)std::strtoull(argv[i], nullptr, 10), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]) != 0, std::atoi(argv[i + 3]), std::atoi(argv[i + 4]), std::atoi(argv[i + 5]));
            std::printf("%zu %zu %zu\n", p.chunk_bytes, p.hungry_min, p.first_bytes);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: map_plan_check devices|pieces|chan ...\n");
    return 2;
}
