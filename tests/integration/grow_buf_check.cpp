// grow_buf_check.cpp -- the contract of mcrc::GrowBuf (memcached_amd/csrc/
// grow_buf.h) over a memory policy that is its own checker: a ledger of live
// blocks at addresses that are never handed out twice, call counts, an
// allocation that can be told to fail, and an abort on the free of any address
// that is not live (a double free, a stale pointer, a foreign pointer).
//
//   g++ -std=c++17 -Wall -Werror -I memcached_amd/csrc grow_buf_check.cpp
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>

#include "grow_buf.h"

namespace {

struct Ledger {
    std::map<void *, size_t> live;
    int allocs = 0, frees = 0, invalid = 0;
    int fail_in = 0;        // k > 0: the k-th allocation from now fails
    bool map_fails = false; // mapped policy: the device view cannot be had
    bool tolerate = false;  // count invalid frees (the negative control) instead of aborting
    uintptr_t next = 0x10000;

    void *alloc(size_t bytes) {
        ++allocs;
        if (fail_in && --fail_in == 0) return nullptr;
        void *p = (void *)next;
        next += (bytes + 0xfff) / 0x1000 * 0x1000 + 0x1000;
        live[p] = bytes;
        return p;
    }
    void free(void *p) {
        ++frees;
        if (live.erase(p)) return;
        if (!tolerate) {
            fprintf(stderr, "free of %p, which is not a live block\n", p);
            abort();
        }
        ++invalid;
    }
} g;

struct FakeMem {
    static bool alloc(size_t bytes, mcrc::Block *b) {
        b->p = b->dv = g.alloc(bytes);
        return b->p != nullptr;
    }
    static void free(const mcrc::Block &b) { g.free(b.p); }
};

// Pinned and mapped: the view is a second step that can fail after the
// allocation succeeded; the policy then frees the block and leaves both
// addresses in *b, as a careless policy would.
constexpr uintptr_t kViewBias = 0x7000000000ull;
struct FakeMapped {
    static bool alloc(size_t bytes, mcrc::Block *b) {
        b->p = g.alloc(bytes);
        if (!b->p) return false;
        b->dv = (void *)((uintptr_t)b->p + kViewBias);
        if (!g.map_fails) return true;
        g.free(b->p);
        return false;
    }
    static void free(const mcrc::Block &b) { g.free(b.p); }
};

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            exit(1);                                                     \
        }                                                                \
    } while (0)

// (every case starts from an empty ledger; buffers have no destructor)
void single_buffer() {
    g = Ledger{};
    mcrc::GrowBuf<FakeMem, uint32_t> b;
    CHECK(b.get() == nullptr && b.bytes() == 0 && b.reserve(0) == nullptr && g.allocs == 0);
    // grow: one allocation of exactly the requested size
    uint32_t *p = b.reserve(1000);
    CHECK(p && p == b.get() && p == b.dev() && b.bytes() == 1000);
    CHECK(g.allocs == 1 && g.frees == 0 && g.live.size() == 1 && g.live.at(p) == 1000);
    // no shrink, no churn
    CHECK(b.reserve(1000) == p && b.reserve(1) == p && b.reserve(0) == p && b.bytes() == 1000);
    CHECK(g.allocs == 1 && g.frees == 0);
    // regrow: the old block freed exactly once and not left live
    uint32_t *q = b.reserve(1001);
    CHECK(q && q != p && b.bytes() == 1001 && g.allocs == 2 && g.frees == 1);
    CHECK(g.live.size() == 1 && g.live.at(q) == 1001);
    // failed regrow: empty, the old block freed once, the next reserve afresh
    g.fail_in = 1;
    CHECK(b.reserve(5000) == nullptr && b.get() == nullptr && b.dev() == nullptr && b.bytes() == 0);
    CHECK(g.allocs == 3 && g.frees == 2 && g.live.empty());
    CHECK(b.reserve(0) == nullptr && g.allocs == 3 && g.frees == 2);
    uint32_t *r = b.reserve(10);  // (smaller than anything before: the buffer really is empty)
    CHECK(r && b.bytes() == 10 && g.allocs == 4 && g.frees == 2 && g.live.size() == 1 && g.live.at(r) == 10);
    // failed first allocation of an empty buffer
    mcrc::GrowBuf<FakeMem> e;
    g.fail_in = 1;
    CHECK(e.reserve(64) == nullptr && e.bytes() == 0 && g.frees == 2 && g.live.size() == 1);
    CHECK(e.reserve(64) != nullptr && g.live.size() == 2);
}

// Ten buffers reserved in sequence, stopping at the first null, as the shim's
// ensure_plan does; every call asks each buffer for more than it holds.  For
// every k: a call whose allocation k fails, then the whole sequence again with
// no failure (so from k = 2 on the failing call starts from ten live blocks).
constexpr int kGroup = 10, kLastRound = 2 * kGroup;
size_t group_size(int i, int round) { return (size_t)(100 + 10 * i) * (size_t)round; }

template <class Reserve>
void group_rounds(Reserve reserve_all) {
    for (int k = 1; k <= kGroup; ++k) {
        g.fail_in = k;
        CHECK(!reserve_all(2 * k - 1));
        CHECK(g.fail_in == 0);
        CHECK(reserve_all(2 * k));
    }
}

void group() {
    g = Ledger{};
    mcrc::GrowBuf<FakeMem> buf[kGroup];
    group_rounds([&](int round) {
        for (int i = 0; i < kGroup; ++i)
            if (!buf[i].reserve(group_size(i, round))) return false;
        return true;
    });
    CHECK(g.invalid == 0 && g.live.size() == kGroup);
    for (int i = 0; i < kGroup; ++i)
        CHECK(buf[i].get() && buf[i].bytes() == group_size(i, kLastRound) &&
              g.live.at(buf[i].get()) == group_size(i, kLastRound));
}

// Negative control: the free-all / allocate-in-one-chain / single-watermark
// scheme the buffers replaced, over the same ledger and the same failures.
// After allocation k fails, the pointers past k still hold freed addresses
// and the next call frees them again.
void group_legacy_scheme_is_caught() {
    g = Ledger{};
    g.tolerate = true;
    void *ptr[kGroup] = {};
    size_t watermark = 0;
    group_rounds([&](int round) {
        if (watermark >= group_size(0, round)) return true;
        for (void *p : ptr)
            if (p) g.free(p);  // (hipFree(nullptr) is a no-op)
        watermark = 0;
        for (int i = 0; i < kGroup; ++i)
            if (!(ptr[i] = g.alloc(group_size(i, round)))) return false;
        watermark = group_size(0, round);
        return true;
    });
    CHECK(g.invalid > 0);
}

void mapped() {
    g = Ledger{};
    mcrc::GrowBuf<FakeMapped, uint8_t> b;
    uint8_t *p = b.reserve(256);
    CHECK(p && b.dev() == p + kViewBias);
    const int frees = g.frees;
    g.map_fails = true;  // the allocation succeeds, the view fails
    CHECK(b.reserve(512) == nullptr && b.get() == nullptr && b.dev() == nullptr && b.bytes() == 0);
    CHECK(g.frees == frees + 2 && g.live.count(p) == 0);  // the old block, and the policy's own new one
    g.map_fails = false;
    g.fail_in = 1;  // the allocation itself fails on an empty buffer
    CHECK(b.reserve(512) == nullptr && b.get() == nullptr && b.dev() == nullptr && g.frees == frees + 2);
    uint8_t *q = b.reserve(512);
    CHECK(q && b.dev() == q + kViewBias && g.live.at(q) == 512);
}

}  // namespace

int main() {
    single_buffer();
    group();
    group_legacy_scheme_is_caught();
    mapped();
    printf("grow_buf ok\n");
    return 0;
}
