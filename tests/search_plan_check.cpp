// search_plan_check.cpp -- stand-alone driver of csrc/ps_search_plan.h for tests/test_search_plan_cpu.py (host compiler, sanitizers on).
//   search_plan_check geometry (<reads> <lm_bytes> <pool_cap> <wide> <cus> <bt_blocks> <max_per_cu> <n_big>)...
//   search_plan_check reserve (<pool_cap> <cus> <bt_blocks> <n_big>)...
//        one line per case: "blocks lanes pool_bytes head_words n_big big_bytes", or "error: <text>"
//   search_plan_check lm (<len> <seed_len> <n_buckets> <wide>)...      one line per case: lm_bytes()
//   search_plan_check knobs                                             defaults, clamps, set / unset / empty; prints "knobs ok"
//   search_plan_check table            per model a line "<name> u0 .. u255", each entry held against budget_diffs() here too
#include <cstdio>
#include <cstring>
#include <string>
#include "ps_search_plan.h"
#include "ps_core.h"
#include "ps_model.h"

using namespace ps;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static void print_plan(const SearchPlan &p) { std::printf("%d %d %zu %zu %u %zu\n", p.blocks, p.lanes, p.pool_bytes, p.head_words, p.n_big, p.big_bytes); }

static const char *KNOBS[] = {"PS_ORDER", "PS_ORDER_MIN", "PS_ORDER_RESTART", "PS_ORDER_WPIN", "PS_ORDER_CAP", "PS_ORDER_SCALE", "PS_MAX_PER_CU",
                              "PS_CAP", "PS_CAP_BIAS", "PS_FETCH_MIN", "PS_HIT_MIN"};
// the knobs with `name` alone set to `value` (nullptr: nothing set)
static SearchKnobs with(const char *name, const char *value, int ctx_fetch_min = 8, int ctx_hit_min = 1)
{
    for (const char *k : KNOBS) unsetenv(k);
    if (name && value) setenv(name, value, 1);
    return search_knobs_from_env(ctx_fetch_min, ctx_hit_min);
}

static int knob_checks()
{
    {   // nothing set: every default
        const SearchKnobs k = with(nullptr, nullptr);
        CHECK(k.order == 1 && k.order_min == 4096 && k.order_restart == 0 && k.order_wpin == 16 && k.order_cap == 255 && k.order_scale == 8);
        CHECK(k.max_per_cu == 4 && k.cap && k.cap_bias == 0 && k.fetch_min == 8 && k.hit_min == 1);
    }
    CHECK(with("PS_ORDER", "0").order == 0); CHECK(with("PS_ORDER", "2").order == 2); CHECK(with("PS_ORDER", "-3").order == -3);      // no clamp
    CHECK(with("PS_ORDER", "").order == 0);
    CHECK(with("PS_ORDER_MIN", "0").order_min == 1); CHECK(with("PS_ORDER_MIN", "-5").order_min == 1); CHECK(with("PS_ORDER_MIN", "1").order_min == 1);
    CHECK(with("PS_ORDER_MIN", "100000").order_min == 100000);
    CHECK(with("PS_ORDER_RESTART", "0").order_restart == 1); CHECK(with("PS_ORDER_RESTART", "-2").order_restart == 1); CHECK(with("PS_ORDER_RESTART", "7").order_restart == 7);
    CHECK(with("PS_ORDER_WPIN", "0").order_wpin == 1); CHECK(with("PS_ORDER_WPIN", "-1").order_wpin == 1); CHECK(with("PS_ORDER_WPIN", "4").order_wpin == 4);
    CHECK(with("PS_ORDER_CAP", "0").order_cap == 1); CHECK(with("PS_ORDER_CAP", "-1").order_cap == 1); CHECK(with("PS_ORDER_CAP", "1").order_cap == 1);
    CHECK(with("PS_ORDER_CAP", "255").order_cap == 255); CHECK(with("PS_ORDER_CAP", "256").order_cap == 255); CHECK(with("PS_ORDER_CAP", "100").order_cap == 100);
    CHECK(with("PS_ORDER_SCALE", "0").order_scale == 1); CHECK(with("PS_ORDER_SCALE", "1").order_scale == 1); CHECK(with("PS_ORDER_SCALE", "12").order_scale == 12);
    CHECK(with("PS_ORDER_SCALE", "13").order_scale == 12); CHECK(with("PS_ORDER_SCALE", "5").order_scale == 5);
    CHECK(with("PS_MAX_PER_CU", "2").max_per_cu == 2); CHECK(with("PS_MAX_PER_CU", "0").max_per_cu == 0); CHECK(with("PS_MAX_PER_CU", "9").max_per_cu == 9);   // no clamp: the plan takes the smaller of it and what the LDS lets in, and refuses less than 1
    // PS_CAP: on unless a value is there that reads as 0 -- the empty string does
    CHECK(with(nullptr, nullptr).cap); CHECK(!with("PS_CAP", "").cap); CHECK(!with("PS_CAP", "0").cap); CHECK(with("PS_CAP", "1").cap);
    CHECK(with("PS_CAP_BIAS", "-1").cap_bias == 0); CHECK(with("PS_CAP_BIAS", "0").cap_bias == 0); CHECK(with("PS_CAP_BIAS", "3").cap_bias == 3);
    CHECK(with("PS_CAP_BIAS", "200").cap_bias == 200); CHECK(with("PS_CAP_BIAS", "201").cap_bias == 200);
    CHECK(with("PS_CAP_BIAS", "3").cap);                          // one knob does not move another
    {   // PS_FETCH_MIN / PS_HIT_MIN: the context reads them when it is made (env_int, unclamped), a search reads them again
        for (const char *name : {"PS_FETCH_MIN", "PS_HIT_MIN"}) {
            const bool fetch = !std::strcmp(name, "PS_FETCH_MIN");
            auto get = [&](const SearchKnobs &k) { return fetch ? k.fetch_min : k.hit_min; };
            for (const char *k : KNOBS) unsetenv(k);
            setenv(name, "3", 1);
            int at_creation = fetch ? 8 : 1;
            CHECK(env_int(name, at_creation) && at_creation == 3);                       // restates Ctx::Ctx (which needs HIP); the real path: tests/test_gpu_repeats.py
            CHECK(get(search_knobs_from_env(fetch ? at_creation : 8, fetch ? 1 : at_creation)) == 3);
            unsetenv(name);                                                              // unset at search time: the context's value holds
            CHECK(get(search_knobs_from_env(fetch ? at_creation : 8, fetch ? 1 : at_creation)) == 3);
            setenv(name, "5", 1);                                                        // set at search time: that wins
            CHECK(get(search_knobs_from_env(fetch ? at_creation : 8, fetch ? 1 : at_creation)) == 5);
            setenv(name, "0", 1); CHECK(get(search_knobs_from_env(3, 3)) == 1);          // clamped below at search time
            setenv(name, "-4", 1); CHECK(get(search_knobs_from_env(3, 3)) == 1);
            setenv(name, "64", 1); CHECK(get(search_knobs_from_env(3, 3)) == 64);        // and not above
            unsetenv(name);
            int untouched = 17;
            CHECK(!env_int(name, untouched) && untouched == 17);
        }
    }
    std::puts("knobs ok");
    return 0;
}

static int table_checks()
{
    const double P[16] = {0.97, 0.01, 0.01, 0.01,  0.01, 0.97, 0.01, 0.01,  0.01, 0.01, 0.97, 0.01,  0.004, 0.12, 0.006, 0.87};
    struct Case { const char *name; Options o; } cases[5];
    cases[0].name = "stock_0.04"; set_stock_n(cases[0].o, "0.04");
    cases[1].name = "stock_2"; set_stock_n(cases[1].o, "2");
    cases[2].name = "profile"; profile_costs(cases[2].o, P, 2.1e-5, 5.9e-4, -1);
    cases[3].name = "profile_X40"; profile_costs(cases[3].o, P, 2.1e-5, 5.9e-4, 40);     // 40 x 8 units: capped
    cases[4].name = "stock_300"; set_stock_n(cases[4].o, "300");
    for (const Case &c : cases) {
        uint8_t tab[256];
        std::memset(tab, 0xAB, sizeof tab);
        budget_units_by_len(c.o, tab);
        std::printf("%s", c.name);
        for (int l = 0; l < 256; ++l) {
            const int u = budget_diffs(c.o, l) * (c.o.profile ? c.o.unit : 1);
            CHECK((int)tab[l] == (u > 255 ? 255 : u));
            std::printf(" %d", (int)tab[l]);
        }
        std::printf("\n");
    }
    CHECK(cases[2].o.profile == 1 && cases[2].o.unit == 8);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "knobs") return knob_checks();
    if (mode == "table") return table_checks();
    if (mode == "lm" && (argc - 2) % 4 == 0) {
        for (int i = 2; i < argc; i += 4) std::printf("%d\n", lm_bytes(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]) != 0));
        return 0;
    }
    if (mode == "geometry" && (argc - 2) % 8 == 0) {
        for (int i = 2; i < argc; i += 8) {
            try {
                print_plan(plan_search(std::atoll(argv[i]), std::atoi(argv[i + 1]), (uint32_t)std::strtoul(argv[i + 2], nullptr, 10), std::atoi(argv[i + 3]) != 0,
                                       std::atoi(argv[i + 4]), std::atoi(argv[i + 5]), std::atoi(argv[i + 6]), std::atoi(argv[i + 7])));
            } catch (const Error &e) { std::printf("error: %s\n", e.what()); }
        }
        return 0;
    }
    if (mode == "reserve" && (argc - 2) % 4 == 0) {
        for (int i = 2; i < argc; i += 4)
            print_plan(plan_search_reserve((uint32_t)std::strtoul(argv[i], nullptr, 10), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3])));
        return 0;
    }
    std::fprintf(stderr, "usage: search_plan_check geometry|reserve|lm|knobs|table ...\n");
    return 2;
}
