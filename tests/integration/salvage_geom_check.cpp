// salvage_geom_check.cpp -- the arithmetic of crc32c_salvage_pages
// (memcached_amd/csrc/salvage_geom.h) run on the CPU: the region cuts the
// kernels make from the walk's lists, the tiles, the header test and the work
// bound.  tests/test_salvage_model.py compares what it prints with the model.
//
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I memcached_amd/csrc salvage_geom_check.cpp
//
//   salvage_geom_check regions W BASE_BYTES BA
//       stdin: "offset covered_end" per list entry (covered_end = offset for
//       an entry that covers nothing), ascending.  Per piece the entries are
//       gone through as k_salvage_regions does (running maximum of the ends,
//       the gap to the next entry or the piece end, salvage_cut), and every
//       range is printed as "r lo hi pe" followed by its tiles "t lo hi".
//       The program itself checks that the tiles partition their range and
//       that none straddles an aligned block.
//   salvage_geom_check span
//       stdin: "nbytes flags nkey cfl room" -> salvage_span per line.
//   salvage_geom_check work
//       stdin: "work scanned wbuf" -> 1 when over the bound, else 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "salvage_geom.h"

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            exit(1);                                                   \
        }                                                              \
    } while (0)

static void emit(uint64_t lo, uint64_t hi, uint64_t pe, uint32_t ba) {
    if (lo >= hi) {
        CHECK(mcrc::salvage_ntiles(lo, hi, ba) == 0);
        return;
    }
    printf("r %llu %llu %llu\n", (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)pe);
    const uint64_t n = mcrc::salvage_ntiles(lo, hi, ba);
    uint64_t at = lo;
    for (uint64_t k = 0; k < n; ++k) {
        const mcrc::SalvageRange t = mcrc::salvage_tile(lo, hi, ba, k);
        CHECK(t.lo == at && t.lo < t.hi && t.hi <= hi);
        CHECK((ba + t.lo) / mcrc::kSalvageTile == (ba + t.hi - 1) / mcrc::kSalvageTile);
        CHECK(k + 1 == n || (ba + t.hi) % mcrc::kSalvageTile == 0);
        printf("t %llu %llu\n", (unsigned long long)t.lo, (unsigned long long)t.hi);
        at = t.hi;
    }
    CHECK(at == hi);
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "span")) {
        unsigned long long nbytes, flags, nkey, cfl, room;
        while (scanf("%llu %llu %llu %llu %llu", &nbytes, &flags, &nkey, &cfl, &room) == 5)
            printf("%u\n", mcrc::salvage_span({(uint32_t)nbytes, (uint32_t)flags, (uint32_t)nkey}, (uint32_t)cfl, room));
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "work")) {
        unsigned long long work, scanned, wbuf;
        while (scanf("%llu %llu %llu", &work, &scanned, &wbuf) == 3)
            printf("%d\n", mcrc::salvage_work_over(work, scanned, wbuf) ? 1 : 0);
        return 0;
    }
    if (argc != 5 || strcmp(argv[1], "regions")) {
        fprintf(stderr, "usage: salvage_geom_check regions W BASE_BYTES BA | span | work\n");
        return 2;
    }
    const uint64_t W = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10);
    const uint32_t ba = (uint32_t)strtoul(argv[4], nullptr, 10);
    CHECK(W > 0 && ba < mcrc::kSalvageTile);
    std::vector<uint64_t> off, end;
    unsigned long long o, e;
    while (scanf("%llu %llu", &o, &e) == 2) {
        CHECK(off.empty() || off.back() < o);
        off.push_back(o);
        end.push_back(e);
    }
    size_t i = 0;
    for (uint64_t w = 0; w * W < n; ++w) {
        const uint64_t ps = w * W, pe = mcrc::salvage_piece_end(w, W, n);
        CHECK(pe > ps && pe <= n && pe - ps <= W);
        uint64_t carry = ps;  // the covered bytes end here
        // the head, then every entry of the piece: the gap behind it
        uint64_t nxt = i < off.size() && off[i] < pe ? off[i] : pe;
        mcrc::SalvageRange r = mcrc::salvage_cut(carry, nxt, ps, pe);
        emit(r.lo, r.hi, pe, ba);
        for (; i < off.size() && off[i] < pe; ++i) {
            if (end[i] > carry) carry = end[i];
            nxt = i + 1 < off.size() && off[i + 1] < pe ? off[i + 1] : pe;
            r = mcrc::salvage_cut(carry, nxt, ps, pe);
            emit(r.lo, r.hi, pe, ba);
        }
    }
    printf("salvage_geom ok\n");
    return 0;
}
