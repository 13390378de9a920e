// k1_slots_check.cpp -- the K1 counter-slot table (memcached_amd/csrc/
// k1_slots.h) driven from 8 threads: one key from all of them, distinct keys,
// more keys than slots, and the special handles.  Plain C++ with its own
// main; tests/test_k1_slots.py builds it plain and with -fsanitize=thread.
//   g++ -std=c++17 -O1 -pthread -I memcached_amd/csrc tests/integration/k1_slots_check.cpp -o k1_slots_check
#include <stdio.h>

#include <set>
#include <thread>
#include <vector>

#include "k1_slots.h"

using mcrc::K1Slots;
using mcrc::kK1Slots;

static int g_fail = 0;
#define EXPECT(c)                                                \
    do {                                                         \
        if (!(c)) {                                              \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail = 1;                                          \
        }                                                        \
    } while (0)

static void *const kLegacy = (void *)1, *const kPerThread = (void *)2;
static void *stream(uintptr_t i) { return (void *)(0x1000 + 64 * i); }
constexpr int kThreads = 8;

template <class F>
static void on_threads(F f) {
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; ++t) th.emplace_back(f, t);
    for (auto &x : th) x.join();
}

int main() {
    {  // the special handles, one thread
        K1Slots s;
        EXPECT(s.find(kPerThread, kLegacy, kPerThread) == -1);
        const int a = s.find(nullptr, kLegacy, kPerThread);
        EXPECT(a >= 0 && a == s.find(kLegacy, kLegacy, kPerThread) && a == s.find(nullptr, kLegacy, kPerThread));
        EXPECT(s.find(stream(0), kLegacy, kPerThread) != a);
        EXPECT(s.find(kPerThread, kLegacy, kPerThread) == -1);
    }
    {  // the same key from every thread: one slot, the same for all, every time
        K1Slots s;
        int got[kThreads];
        on_threads([&](int t) {
            int first = s.find(stream(7), kLegacy, kPerThread);
            for (int i = 0; i < 10000; ++i)
                if (s.find(stream(7), kLegacy, kPerThread) != first) first = -2;
            got[t] = first;
        });
        for (int t = 0; t < kThreads; ++t) EXPECT(got[t] == got[0] && got[0] >= 0);
        int used = 0;
        for (auto &k : s.key) used += k.load() != 0;
        EXPECT(used == 1);
    }
    {  // distinct keys, the null / legacy pair among them: distinct slots, stable on a second look
        K1Slots s;
        int got[kThreads][4], again[kThreads][4];
        on_threads([&](int t) {
            for (int j = 0; j < 4; ++j) {
                void *k = t == 0 && j == 0 ? nullptr : t == 1 && j == 0 ? kLegacy : stream(4 * t + j);
                got[t][j] = s.find(k, kLegacy, kPerThread);
            }
            for (int j = 0; j < 4; ++j) {
                void *k = t == 0 && j == 0 ? kLegacy : t == 1 && j == 0 ? nullptr : stream(4 * t + j);
                again[t][j] = s.find(k, kLegacy, kPerThread);
            }
        });
        std::set<int> slots;
        for (int t = 0; t < kThreads; ++t)
            for (int j = 0; j < 4; ++j) {
                EXPECT(got[t][j] >= 0 && got[t][j] == again[t][j]);
                slots.insert(got[t][j]);
            }
        EXPECT(got[0][0] == got[1][0]);  // null and the legacy handle
        EXPECT(slots.size() == 4 * kThreads - 1);
    }
    {  // more keys than slots: kK1Slots of them get distinct slots, the rest none, and that stays so
        K1Slots s;
        constexpr int per = (kK1Slots + 2 + kThreads - 1) / kThreads + 4;
        int got[kThreads][per];
        on_threads([&](int t) {
            for (int j = 0; j < per; ++j) got[t][j] = s.find(stream(per * t + j), kLegacy, kPerThread);
        });
        std::set<int> slots;
        int none = 0;
        for (int t = 0; t < kThreads; ++t)
            for (int j = 0; j < per; ++j) {
                if (got[t][j] < 0) ++none;
                else EXPECT(slots.insert(got[t][j]).second);
                EXPECT(s.find(stream(per * t + j), kLegacy, kPerThread) == got[t][j]);
            }
        EXPECT((int)slots.size() == kK1Slots && none == kThreads * per - kK1Slots);
        EXPECT(s.find(nullptr, kLegacy, kPerThread) == -1);
    }
    printf(g_fail ? "FAILED\n" : "ok\n");
    return g_fail;
}
