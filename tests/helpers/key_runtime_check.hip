// TEST HELPER (stand-alone host program, no GPU): the runtime state both keys hold (csrc/key_runtime.hpp: mutex, per-ctx arenas,
// count of running calls, retire) and the ctx serial numbers it is filed under (csrc/ctx.hpp), driven directly.  Arenas without
// blocks never reach the HIP runtime, so nothing here needs a device.  tests/test_key_runtime_cpu.py builds it with the host's
// address and undefined-behaviour sanitizers (and, where it links, the thread sanitizer) and runs it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "ctx.hpp"
namespace bzh {
namespace {
#include "key_runtime.hpp"
}  // namespace
}  // namespace bzh
using bzh::KeyRuntime;

static int bad = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAIL line %d: %s\n", __LINE__, #cond);              \
            bad++;                                                      \
        }                                                               \
    } while (0)

static int count_of(KeyRuntime& rt) {
    std::lock_guard<std::mutex> lk(rt.mu);
    return rt.calls;
}

// retire() refuses while a guard is alive, touching nothing, and succeeds once it is gone
static void guard_then_retire() {
    KeyRuntime rt;
    bzh::Arena* a = &rt.arena_for(7, 0);
    {
        KeyRuntime::Call outer(rt);
        CHECK(count_of(rt) == 1);
        {
            KeyRuntime::Call inner(rt);
            CHECK(count_of(rt) == 2 && !rt.retire());
        }
        CHECK(count_of(rt) == 1 && !rt.retire());
        CHECK(rt.arenas.size() == 1 && &rt.arena_for(7, 0) == a);   // a refusal leaves the arenas where they are
    }
    CHECK(count_of(rt) == 0);
    CHECK(rt.retire() && rt.arenas.empty() && count_of(rt) == 0);
}

// serials: distinct over threads and over contexts created one after the other at (possibly) the same address
static void serials() {
    constexpr int T = 4, N = 2000;
    std::vector<std::vector<uint64_t>> got(T);
    std::vector<std::thread> ths;
    for (int t = 0; t < T; t++)
        ths.emplace_back([&, t] {
            for (int i = 0; i < N; i++) {
                std::unique_ptr<bzh_ctx> c(new bzh_ctx());   // freed at once: the next one often gets the address back
                got[t].push_back(c->serial);
            }
        });
    for (auto& th : ths) th.join();
    std::vector<uint64_t> all;
    for (auto& g : got) all.insert(all.end(), g.begin(), g.end());
    std::sort(all.begin(), all.end());
    CHECK(all.size() == (size_t)T * N && std::adjacent_find(all.begin(), all.end()) == all.end() && all.front() != 0);
    bzh_ctx x, y;
    CHECK(x.serial != y.serial);
}

// arena_for: one arena per serial, kept; a ctx created after another one was destroyed gets a fresh arena on its own device
static void arenas() {
    KeyRuntime rt;
    bzh_ctx* a = new bzh_ctx();
    a->device = 0;
    const uint64_t sa = a->serial;
    bzh::Arena* aa = &rt.arena_for(a->serial, a->device);
    CHECK(&rt.arena_for(a->serial, a->device) == aa && aa->device == 0 && rt.arenas.size() == 1);
    delete a;
    bzh_ctx* b = new bzh_ctx();   // the allocator may hand the same address out again
    b->device = 1;
    bzh::Arena* ab = &rt.arena_for(b->serial, b->device);
    CHECK(b->serial != sa && ab != aa && ab->device == 1 && aa->device == 0 && rt.arenas.size() == 2);
    CHECK(&rt.arena_for(sa, 0) == aa && &rt.arena_for(b->serial, 1) == ab && rt.arenas.size() == 2);   // the old one stays until the key goes
    {
        std::lock_guard<std::mutex> lk(rt.mu);
        CHECK(rt.held_locked() == 0);
    }
    delete b;
    CHECK(rt.retire() && rt.arenas.empty());
}

// Eight threads open and close guards while a ninth keeps asking to retire.  The owner of the key holds a guard of its own
// until the workers are joined (the contract of include/bzh2.h: no call starts after a free that went through), so: every
// refusal comes while a guard is alive, the one success after the last is gone, and nothing touches the runtime after it.
static void threads() {
    constexpr int T = 8, N = 10000;
    KeyRuntime rt;
    (void)rt.arena_for(1, 0);
    (void)rt.arena_for(2, 0);
    std::atomic<bool> dropping{false}, dropped{false};
    std::atomic<int> wrong{0};
    std::atomic<long> refusals{0}, successes{0};
    std::unique_ptr<KeyRuntime::Call> owner(new KeyRuntime::Call(rt));
    std::vector<std::thread> workers;
    for (int t = 0; t < T; t++)
        workers.emplace_back([&] {
            for (int i = 0; i < N; i++) {
                KeyRuntime::Call c(rt);
                if (count_of(rt) < 2) wrong++;   // this guard and the owner's
                if ((i & 1023) == 0) (void)rt.arena_for(100 + (uint64_t)i, 0);   // the map grows under the same mutex
            }
        });
    std::thread freer([&] {
        for (;;) {
            const bool none_before = dropped.load();   // read BEFORE the attempt: true = the count was zero throughout it
            if (rt.retire()) {
                successes++;
                if (!dropping.load()) wrong++;   // went through while the owner's guard was certainly alive
                return;                          // nothing is touched after the success
            }
            refusals++;
            if (none_before) wrong++;            // refused with no guard alive
            std::this_thread::yield();
        }
    });
    for (auto& th : workers) th.join();
    CHECK(count_of(rt) == 1);
    while (refusals.load() == 0) std::this_thread::yield();   // (the owner's guard is alive: the next attempt is a refusal)
    dropping = true;
    owner.reset();
    dropped = true;
    freer.join();
    CHECK(wrong.load() == 0 && successes.load() == 1 && refusals.load() >= 1);
    CHECK(rt.calls == 0 && rt.arenas.empty());
    printf("%d guards, %ld refusals, %ld success\n", T * N, refusals.load(), successes.load());
}

int main(int argc, char** argv) {
    const bool threads_only = argc > 1 && std::string(argv[1]) == "threads";
    if (!threads_only) {
        guard_then_retire();
        serials();
        arenas();
    }
    threads();
    if (bad) return 1;
    printf("key_runtime_check: ok\n");
    return 0;
}
