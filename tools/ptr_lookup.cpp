// ptr_lookup.cpp -- what one span's lookup in the registry of page-locked
// ranges (memcached_amd/csrc/host_route.h PinRegistry::view) costs, on the host
// alone: batches of 64 lookups at random places of R recorded ranges.
//
//   g++ -O2 -std=c++17 -I memcached_amd/csrc tools/ptr_lookup.cpp -o ptr_lookup && ./ptr_lookup
//
// Prints one JSON object: ns per lookup for R = 1, 64 and 4096.
#include <stdint.h>
#include <stdio.h>

#include <chrono>
#include <vector>

#include "host_route.h"

int main() {
    printf("{");
    for (const uint64_t ranges : {1ull, 64ull, 4096ull}) {
        mcrc::PinRegistry reg;
        const uint64_t page = 1ull << 20;
        for (uint64_t r = 0; r < ranges; ++r)  // 1 MiB pages, 1 MiB apart
            reg.record((const void *)(uintptr_t)((2 * r + 1) * page), page, (const void *)(uintptr_t)(r * page));
        uint64_t rng = 88172645463325252ull, sink = 0;
        std::vector<const void *> spans(64);
        const int batches = 20000;
        double ns = 0;
        for (int b = 0; b < batches; ++b) {
            for (auto &p : spans) {
                rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
                p = (const void *)(uintptr_t)((2 * (rng % ranges) + 1) * page + (rng >> 20) % (page - 4133));
            }
            const auto t0 = std::chrono::steady_clock::now();
            for (const void *p : spans) {
                const uint8_t *dv = nullptr;
                sink += reg.view(p, 4133, &dv) == mcrc::PinRegistry::Hit::inside ? (uintptr_t)dv : 1;
            }
            ns += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
        }
        printf("%s\"ranges_%llu_ns_per_span\": %.1f", ranges == 1 ? "" : ", ", (unsigned long long)ranges,
               ns / (64.0 * batches));
        if (sink == 42) printf(" ");
    }
    printf("}\n");
    return 0;
}
