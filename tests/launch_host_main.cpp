// Stand-alone CPU program around csrc/amt_launch_core.h, the book-keeping of a kernel launch: built by
// tests/test_launch_core_cpu.py with the address and undefined-behaviour sanitizers and again with the thread sanitizer.
// A fake setter stands where amt_launch.h calls the runtime; it counts and records its calls.
//
//   launch_host_main        exit 0 and "ok" if every check holds, else the failed check on stderr and exit 1
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "amt_launch_core.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static void six_guarantees() {
    amt_lds_limits lim;
    std::vector<size_t> calls;
    int fail_next = 0;
    auto set = [&](size_t bytes) { calls.push_back(bytes); return fail_next ? fail_next : 0; };
    int fa = 0, fb = 0;                                            // two function keys
    // 1. the first request for a key calls the setter with the bytes wanted
    CHECK(lim.request(0, &fa, 1000, set) == 0 && calls == std::vector<size_t>{1000});
    // 2. at or below the record: nothing
    CHECK(lim.request(0, &fa, 1000, set) == 0 && lim.request(0, &fa, 1, set) == 0 && calls.size() == 1);
    // 3. a larger request calls it with the new value, and the record has grown
    CHECK(lim.request(0, &fa, 1001, set) == 0 && calls.size() == 2 && calls.back() == 1001);
    CHECK(lim.request(0, &fa, 1001, set) == 0 && calls.size() == 2);
    // 4. devices (and functions) are independent
    CHECK(lim.request(1, &fa, 10, set) == 0 && calls.size() == 3 && calls.back() == 10);
    CHECK(lim.request(0, &fb, 10, set) == 0 && calls.size() == 4 && calls.back() == 10);
    CHECK(lim.request(0, &fa, 1001, set) == 0 && lim.request(1, &fa, 10, set) == 0 && calls.size() == 4);
    // 5. a failing setter: its status comes back, the record stays, the next request tries again
    fail_next = -3;
    CHECK(lim.request(0, &fa, 5000, set) == -3 && calls.size() == 5 && calls.back() == 5000);
    CHECK(lim.request(0, &fa, 1001, set) == 0 && calls.size() == 5);           // (what was granted before still is)
    CHECK(lim.request(2, &fa, 64, set) == -3 && calls.size() == 6);            // a first request that fails records nothing
    fail_next = 0;
    CHECK(lim.request(0, &fa, 5000, set) == 0 && calls.size() == 7 && calls.back() == 5000);
    CHECK(lim.request(2, &fa, 64, set) == 0 && calls.size() == 8 && calls.back() == 64);
    CHECK(lim.request(0, &fa, 5000, set) == 0 && lim.request(2, &fa, 64, set) == 0 && calls.size() == 8);
}

// 6. concurrent requests: 8 threads, 2 devices, 3 functions, mixed sizes.  A caller returns only after the limit is at
// least what it asked for; the setter never sees a value below one already granted; at the end every key's limit is
// the largest request for it.
static void concurrent_requests() {
    const int THREADS = 8, DEVICES = 2, FUNCS = 3, REQUESTS = 4000;
    amt_lds_limits lim;
    int fn[FUNCS] = {0, 0, 0};
    std::atomic<size_t> granted[DEVICES][FUNCS], largest[DEVICES][FUNCS];
    for (auto &d : granted) for (auto &g : d) g = 0;
    for (auto &d : largest) for (auto &g : d) g = 0;
    std::atomic<int> bad{0}, calls{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; ++t) {
        pool.emplace_back([&, t] {
            unsigned s = 0x9E3779B9u * (unsigned)(t + 1);
            for (int i = 0; i < REQUESTS; ++i) {
                s = s * 1664525u + 1013904223u;
                const int d = (s >> 8) % DEVICES, f = (s >> 12) % FUNCS;
                const size_t want = 1 + (s >> 16) % (160 * 1024);
                size_t seen = largest[d][f].load();
                while (seen < want && !largest[d][f].compare_exchange_weak(seen, want)) {}
                const int rc = lim.request(d, &fn[f], want, [&](size_t bytes) {
                    ++calls;
                    if (bytes != want || bytes <= granted[d][f].load()) ++bad;       // never at or below what is granted
                    granted[d][f].store(bytes);
                    return 0;
                });
                if (rc != 0 || granted[d][f].load() < want) ++bad;
            }
        });
    }
    for (auto &th : pool) th.join();
    CHECK(bad == 0);
    CHECK(calls >= DEVICES * FUNCS && calls < THREADS * REQUESTS);
    for (int d = 0; d < DEVICES; ++d)
        for (int f = 0; f < FUNCS; ++f) {
            CHECK(largest[d][f] > 0 && granted[d][f] == largest[d][f]);
            const int before = calls;
            CHECK(lim.request(d, &fn[f], largest[d][f], [&](size_t) { ++calls; return 0; }) == 0 && calls == before);
        }
}

static void environment() {
    const char *name = "AMT_LAUNCH_HOST_MAIN";
    struct { const char *text; bool on; long number, from0; } cases[] = {
        {nullptr, true, 7, 7}, {"", true, 7, 7}, {"0", false, 7, 0}, {"1", true, 1, 1}, {"00", false, 7, 0},
        {"16", true, 16, 16}, {"-3", true, 7, 7}, {"abc", true, 7, 7}};
    for (const auto &c : cases) {
        if (c.text) setenv(name, c.text, 1); else unsetenv(name);
        CHECK(amt_env_switch(name, true) == c.on);
        CHECK(amt_env_switch(name, false) == (c.text ? c.on : false));       // unset: the default, whichever it is
        CHECK(amt_env_number(name, 7) == c.number);                          // positive, or the default
        CHECK(amt_env_number(name, 7, 0) == c.from0);                        // ... where zero is a value too
    }
    unsetenv(name);
}

static void hop_shift() {
    struct { int hop; bool ok; int shift; } cases[] = {{64, false, -1}, {128, true, 7}, {129, false, -1}, {2048, true, 11},
                                                       {4096, false, -1}, {0, false, -1}, {-128, false, -1}};
    for (const auto &c : cases) {
        int shift = -1;
        CHECK(amt_hop_shift(c.hop, 128, 2048, &shift) == c.ok && shift == c.shift);
    }
}

int main() {
    six_guarantees();
    concurrent_requests();
    environment();
    hop_shift();
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
