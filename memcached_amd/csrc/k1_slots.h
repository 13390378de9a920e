// k1_slots.h -- which counter slot (K1Ctl, k_consts.h) a K1 launch on a given
// stream uses.  K1 is launched from many threads and streams without the
// device's mutex, so the counters are per stream: launches on one stream run
// one after another and the kernel leaves its slot zeroed, which is the whole
// safety argument.  A fixed table keyed by the stream handle; lookups take no
// lock, an insert is one compare-and-swap, entries are never removed (a
// handle the runtime hands out again for a later stream keeps its slot).
// Plain C++, no HIP include: the handle is a void *, the special handles are
// the caller's; tests/integration/k1_slots_check.cpp drives it from threads.
#pragma once

#include <stdint.h>

#include <atomic>

namespace mcrc {

constexpr int kK1Slots = 64;

struct K1Slots {
    std::atomic<uintptr_t> key[kK1Slots];
    K1Slots() {
        for (auto &k : key) k.store(0, std::memory_order_relaxed);
    }
    // The slot of `stream`, or -1 for none (the launch is then the static
    // K1: slower at worst).  The null stream and `legacy` (the legacy default
    // handle, not null) are one stream and share a key; `per_thread` stands
    // for one stream per host thread under one handle, so it never gets a slot;
    // so does every stream once the table is full.
    int find(void *stream, void *legacy, void *per_thread) {
        if (stream == per_thread) return -1;
        const uintptr_t k = stream ? (uintptr_t)stream : (uintptr_t)legacy;
        for (int i = 0; i < kK1Slots; ++i) {
            uintptr_t cur = key[i].load(std::memory_order_acquire);
            if (cur == 0 && key[i].compare_exchange_strong(cur, k, std::memory_order_acq_rel)) return i;
            if (cur == k) return i;  // (found, or another thread has just inserted this stream here)
        }
        return -1;
    }
};

}  // namespace mcrc
