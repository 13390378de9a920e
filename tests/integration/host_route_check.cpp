// host_route_check.cpp -- the host shim's decisions (memcached_amd/csrc/
// host_route.h) run on the CPU for every shape at which they change: the
// routes of span and item batches, the launch geometry, the plan's rounds and
// capacity, the host pipeline's staging order and chunk cuts, the shard cuts.
// No pointer of a batch is ever dereferenced by a route, so the batches here
// carry made-up addresses.
//
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I memcached_amd/csrc host_route_check.cpp
//
//   host_route_check             every assertion; prints the fixed-length K5 and
//                                k_blocks sets ("k5 <len>..." / "blocks <len>...")
//   host_route_check cuts PARTS  span lengths on stdin -> crc32c_shard_cuts' cut points
//   host_route_check route N LEN STRIDE OFFSETS LENS BASE_MOD BASE_BYTES SMALL_MAX
//                                the name of span_route's answer for that batch
//                                (OFFSETS / LENS: 1 when the array is given)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "host_route.h"

namespace {

using mcrc::ItemRoute;
using mcrc::SpanRoute;

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            exit(1);                                                   \
        }                                                              \
    } while (0)

const uint64_t *const kSomeOffsets = (const uint64_t *)0x1000;  // (given or not: never read)
const uint32_t *const kSomeLens = (const uint32_t *)0x2000;
constexpr uint64_t kSmallMax = mcrc_dev::kSmallMax;

crc32c_spans fixed(uint64_t n, uint32_t len, bool offsets, uintptr_t base = 0x7f0000000000ull,
                   uint64_t stride = 16384) {
    crc32c_spans s{};
    s.base = (const void *)base;
    s.base_bytes = 1ull << 50;
    s.offsets = offsets ? kSomeOffsets : nullptr;
    s.stride = stride;
    s.len = len;
    s.n = n;
    return s;
}

void fixed_length_routes() {
    const uint64_t n = 8193;  // one past the largest small batch
    std::vector<uint32_t> k5, blocks;
    for (int offsets = 0; offsets < 2; ++offsets)
        for (uint32_t len = 0; len <= 9000; ++len) {
            // (without offsets: a base that is not 16-B aligned, so 4096 is not K1's)
            const SpanRoute r = mcrc::span_route(fixed(n, len, offsets, 0x7f0000000008ull), kSmallMax);
            CHECK((r == SpanRoute::k5) == (len >= 4099 && len <= 4227));
            CHECK((r == SpanRoute::id_blocks) == (len >= 4081 && len <= 4097));
            if (len + 127 <= 512) CHECK(r == SpanRoute::id_final);  // no k_spans launch
            else if (r != SpanRoute::k5 && r != SpanRoute::id_blocks) CHECK(r == SpanRoute::id_spans);
            if (offsets && r == SpanRoute::k5) k5.push_back(len);
            if (offsets && r == SpanRoute::id_blocks) blocks.push_back(len);
        }
    CHECK(k5.size() == 129 && blocks.size() == 17);
    printf("k5");
    for (uint32_t l : k5) printf(" %u", l);
    printf("\nblocks");
    for (uint32_t l : blocks) printf(" %u", l);
    printf("\n");
    // K1: 4096-B spans, no offsets, a 16-B aligned base and stride below 2^31
    for (uint32_t len = 0; len <= 9000; ++len)
        CHECK((mcrc::span_route(fixed(n, len, false), kSmallMax) == SpanRoute::k1) == (len == 4096));
    CHECK(mcrc::span_route(fixed(n, 4096, true), kSmallMax) != SpanRoute::k1);
    CHECK(mcrc::span_route(fixed(n, 4096, false, 0x7f0000000008ull), kSmallMax) != SpanRoute::k1);
    CHECK(mcrc::span_route(fixed(n, 4096, false, 0x7f0000000000ull, 4104), kSmallMax) != SpanRoute::k1);
    CHECK(mcrc::span_route(fixed(n, 4096, false, 0x7f0000000000ull, (1ull << 31) - 16), kSmallMax) == SpanRoute::k1);
    CHECK(mcrc::span_route(fixed(2, 4096, false, 0x7f0000000000ull, 1ull << 31), kSmallMax) != SpanRoute::k1);
    CHECK(mcrc::span_route(fixed(1, 4096, false), kSmallMax) == SpanRoute::k1);  // (K1 comes before small)
    crc32c_spans v = fixed(n, 4096, false);
    v.lens = kSomeLens;
    CHECK(mcrc::span_route(v, kSmallMax) == SpanRoute::planned);
    // empty and rejected batches
    CHECK(mcrc::span_route(fixed(0, 4096, false), kSmallMax) == SpanRoute::empty);
    crc32c_spans o = fixed(4, 4096, false);
    o.base_bytes = 3 * 16384 + 4095;  // the last span overruns by a byte
    CHECK(mcrc::span_route(o, kSmallMax) == SpanRoute::invalid);
    o.base_bytes += 1;
    CHECK(mcrc::span_route(o, kSmallMax) == SpanRoute::k1);
    CHECK(mcrc::span_route(fixed(n, mcrc_dev::kMaxSpan + 1, true), kSmallMax) == SpanRoute::invalid);
    CHECK(mcrc::span_route(fixed(n, mcrc_dev::kMaxSpan, true), kSmallMax) == SpanRoute::planned);
    CHECK(mcrc::span_route(fixed(n, mcrc_dev::kSegBytes, true), kSmallMax) == SpanRoute::id_spans);
    CHECK(mcrc::span_route(fixed(n, mcrc_dev::kSegBytes + 1, true), kSmallMax) == SpanRoute::planned);
    // 2^32 - 1 spans: no K5, no plan; the identity kernels index in 64 bits
    CHECK(mcrc::span_route(fixed(0xffffffffull, 4133, true), kSmallMax) == SpanRoute::id_spans);
    CHECK(mcrc::span_route(fixed(0xfffffffeull, 4133, true), kSmallMax) == SpanRoute::k5);
    v.n = 0xffffffffull;
    CHECK(mcrc::span_route(v, kSmallMax) == SpanRoute::invalid);
    v.n = 0xfffffffeull;
    CHECK(mcrc::span_route(v, kSmallMax) == SpanRoute::planned);
}

void small_rule() {
    for (uint64_t small_max : {(uint64_t)0, (uint64_t)64, kSmallMax})
        for (uint64_t n : {(uint64_t)1, small_max, small_max + 1}) {
            if (n == 0) continue;
            // fixed length: spans of at most 1 MiB, whatever the buffer
            CHECK((mcrc::span_route(fixed(n, 1 << 20, true), small_max) == SpanRoute::small) == (n <= small_max));
            CHECK(mcrc::span_route(fixed(n, (1 << 20) + 1, true), small_max) == SpanRoute::planned);
            // lengths given: a buffer of at most 8 MiB
            crc32c_spans v = fixed(n, 0, true);
            v.lens = kSomeLens;
            v.base_bytes = 8ull << 20;
            CHECK(mcrc::span_route(v, small_max) == (n <= small_max ? SpanRoute::small : SpanRoute::planned));
            v.base_bytes += 1;
            CHECK(mcrc::span_route(v, small_max) == SpanRoute::planned);
            // items: as lengths given
            CHECK(mcrc::item_route(n, 8ull << 20, small_max) ==
                  (n <= small_max ? ItemRoute::small : n >= 4096 ? ItemRoute::k5 : ItemRoute::planned));
            CHECK(mcrc::item_route(n, (8ull << 20) + 1, small_max) != ItemRoute::small);
        }
}

void item_routes() {
    const uint64_t big = 1ull << 30;
    CHECK(mcrc::item_route(4095, big, kSmallMax) == ItemRoute::planned);
    CHECK(mcrc::item_route(4096, big, kSmallMax) == ItemRoute::k5);
    CHECK(mcrc::item_route(4096, big, kSmallMax, false) == ItemRoute::planned);  // staged images of a stamp
    CHECK(mcrc::item_route(4096, 8ull << 20, kSmallMax) == ItemRoute::small);    // small comes first
    CHECK(mcrc::item_route(4096, 8ull << 20, 0) == ItemRoute::k5);
    CHECK(mcrc::item_route(0xfffffffeull, big, kSmallMax) == ItemRoute::k5);
    CHECK(mcrc::item_route(0xffffffffull, big, kSmallMax) == ItemRoute::invalid);
    CHECK(mcrc::item_route(0xffffffffull, big, kSmallMax, false) == ItemRoute::invalid);
}

void geometry() {
    for (int cus : {1, 8, 256})
        for (uint64_t n = 1; n <= 8192; ++n) {
            const uint64_t per = mcrc::small_per(cus, n), groups = (n + per - 1) / per;  // (as launch_small)
            CHECK(per % 2 == 0 && per >= 8 && per <= 32);
            CHECK(groups * per >= n && (groups - 1) * per < n);
            // (never fewer workgroups than one span per 32-lane group of a full workgroup gives, up to a CU each)
            CHECK(groups >= std::min<uint64_t>(cus, (n + 31) / 32));
            const int grid = mcrc::grid_for(cus, n);
            CHECK(grid >= 1 && grid <= cus && (grid == cus || (uint64_t)grid * 32 >= n));
            const uint32_t nsr = mcrc::k5_nsr(grid, n);
            CHECK(nsr >= 1 && nsr <= mcrc_dev::kEpoch);
        }
    CHECK(mcrc::small_per(0, 100) == 32);  // (a device that reports no CUs)
    CHECK(mcrc::grid_for(256, 0) == 1);
    CHECK(mcrc::count_grid(1) == 1 && mcrc::count_grid(2048 * 256 + 1) == 2048);
    CHECK(mcrc::final_grid(257) == 2 && mcrc::final_grid(1 << 30) == 1024);
    CHECK(mcrc::plan_tiles(2048) == 1 && mcrc::plan_tiles(2049) == 2 && mcrc::plan_tile_grid(1ull << 40) == 4096);
    CHECK(mcrc::span_groups(256) == 256 * 32);
    CHECK(mcrc::plan_rounds(0) == 1 && mcrc::plan_rounds(8ull << 30) == 1 && mcrc::plan_rounds((8ull << 30) + 1) == 2);
    CHECK(mcrc::plan_rounds(128ull << 30) == 16 && mcrc::plan_rounds(1ull << 60) == 16);
    uint64_t last = 0;
    for (uint64_t n = 0; n < (1ull << 33); n = n * 3 + 1)
        for (uint64_t bytes = 0; bytes < (1ull << 50); bytes = bytes * 5 + 4096) {
            const uint64_t cap = mcrc::plan_cap(n, bytes);
            CHECK(cap <= 0xfffffff0ull && cap >= std::min<uint64_t>(n, 0xfffffff0ull));
            CHECK(cap >= mcrc::plan_cap(n, bytes / 5) && cap >= mcrc::plan_cap(n / 3, bytes));  // monotone
            last = std::max(last, cap);
        }
    CHECK(last == 0xfffffff0ull);
    CHECK(mcrc::walk_grid(1) == 1 && mcrc::walk_grid(5) == 2 && mcrc::walk_grid(1ull << 30) == 65535);
    CHECK(mcrc::walk_kslot(4ull << 20) == 2048 && mcrc::walk_kslot(16383) == 0 && mcrc::walk_kslot(16384) == 8);
    CHECK(mcrc::walk_kslot(1ull << 40) == 8192);
}

// Every span in exactly one chunk, each chunk within its limits, the scatter
// order the inverse of the staging order.
void check_cuts(const std::vector<uint64_t> &offs, const std::vector<uint32_t> &lens, uint64_t slot_bytes,
                uint64_t slot_items, size_t want_chunks = 0) {
    crc32c_spans s{};
    s.base_bytes = ~0ull;
    s.offsets = offs.data();
    s.lens = lens.data();
    s.n = offs.size();
    CHECK(mcrc::host_spans_ok(s, slot_bytes));
    const std::vector<uint64_t> order = mcrc::staging_order(s);
    bool sorted = true;
    for (size_t i = 1; i < offs.size(); ++i) sorted = sorted && offs[i - 1] <= offs[i];
    CHECK(order.empty() == sorted);
    std::vector<int> seen(s.n, 0);
    std::vector<uint64_t> staged;  // caller index of each staging position, as the pipeline walks them
    size_t chunks = 0;
    for (uint64_t k0 = 0; k0 < s.n; ++chunks) {
        const mcrc::Chunk c = mcrc::next_chunk(s, order, k0, slot_bytes, slot_items);
        CHECK(c.k1 > k0 && c.k1 - k0 <= slot_items && c.hi - c.lo <= slot_bytes && (c.lo & 15u) == 0);
        for (uint64_t k = k0; k < c.k1; ++k) {
            const uint64_t i = order.empty() ? k : order[k];
            CHECK(offs[i] >= c.lo && offs[i] + lens[i] <= c.hi);
            if (k > 0) CHECK(offs[order.empty() ? k - 1 : order[k - 1]] <= offs[i]);  // offset order
            ++seen[i];
            staged.push_back(i);
        }
        k0 = c.k1;
    }
    for (int v : seen) CHECK(v == 1);
    // The staging order against a sort of its own: (offset, caller index) pairs in plain
    // lexicographic order are the stable order by offset.  Scattering as run_host_batch does
    // (out[staged[k]] = result k, result k being that of the k-th pair) must then put every
    // span's own result at its caller index.
    std::vector<std::pair<uint64_t, uint64_t>> want(s.n);
    for (uint64_t i = 0; i < s.n; ++i) want[i] = {offs[i], i};
    std::sort(want.begin(), want.end());
    std::vector<uint64_t> out(s.n, ~0ull);
    for (uint64_t k = 0; k < s.n; ++k) out[staged[k]] = want[k].second;
    for (uint64_t i = 0; i < s.n; ++i) CHECK(out[i] == i);
    if (want_chunks) CHECK(chunks == want_chunks);
}

void pipeline_cuts() {
    const uint64_t SB = mcrc::kSlotBytes, SI = mcrc::kSlotItems;
    // the largest span a slot takes, at an unaligned offset: a chunk of its own
    // between two small ones; and a span that alone forces a cut
    check_cuts({7, 100, 100 + SB - 16 + 9, 2 * SB + 5, 2 * SB + 1000},
               {50, (uint32_t)(SB - 16), 30, 64, (uint32_t)(SB - 1200)},
               SB, SI, 4);
    check_cuts({15}, {(uint32_t)(SB - 16)}, SB, SI, 1);
    crc32c_spans big{};
    const uint64_t off = 0;
    const uint32_t len = (uint32_t)(SB - 15);
    big.base_bytes = ~0ull;
    big.offsets = &off;
    big.lens = &len;
    big.n = 1;
    CHECK(!mcrc::host_spans_ok(big));  // (one byte more than a slot takes at any alignment)
    big.base_bytes = len - 1;
    CHECK(!mcrc::host_spans_ok(big));
    // small slots, sorted and unsorted lists, overlapping and equal offsets, the item limit
    uint64_t x = 12345;
    auto rnd = [&] { return (x = x * 6364136223846793005ull + 1442695040888963407ull) >> 33; };
    for (int round = 0; round < 200; ++round) {
        const size_t n = 1 + rnd() % 300;
        std::vector<uint64_t> offs(n);
        std::vector<uint32_t> lens(n);
        uint64_t at = rnd() % 64;
        for (size_t i = 0; i < n; ++i) {
            lens[i] = (uint32_t)(rnd() % (round % 3 ? 700 : 4096 - 16 + 1));
            offs[i] = at;
            at += rnd() % 4 ? rnd() % 900 : 0;
        }
        if (round % 2)
            for (size_t i = n - 1; i > 0; --i) {
                const size_t j = rnd() % (i + 1);
                std::swap(offs[i], offs[j]);
                std::swap(lens[i], lens[j]);
            }
        check_cuts(offs, lens, 4096, 1 + round % 7);
    }
    // the chain fold's staging buffer: the parts in order, disjoint, aligned, inside the buffer
    for (uint64_t n : {0ull, 1ull, 7ull, 1000ull})
        for (uint64_t nchains : {1ull, 2ull, 333ull}) {
            const uint64_t first = mcrc::chain_first_off(n), out = first + (nchains + 1) * 8;  // (as the chain call)
            CHECK(2 * n * 4 <= first && first < 2 * n * 4 + 8 && first % 8 == 0);
            CHECK(out + nchains * 4 <= mcrc::chain_stage_bytes(n, nchains));
        }
    CHECK(mcrc::ranges_overlap((void *)100, 10, (void *)109, 5));
    CHECK(!mcrc::ranges_overlap((void *)100, 10, (void *)110, 5));
    CHECK(!mcrc::ranges_overlap((void *)100, 0, (void *)100, 5));
    CHECK(mcrc::ranges_overlap((void *)105, 1, (void *)100, 10));
}

int print_cuts(int parts) {
    std::vector<uint32_t> lens;
    unsigned long v;
    while (scanf("%lu", &v) == 1) lens.push_back((uint32_t)v);
    std::vector<uint64_t> cuts(parts + 1);
    mcrc::shard_cuts(lens.data(), 0, lens.size(), parts, cuts.data());
    for (uint64_t c : cuts) printf("%llu ", (unsigned long long)c);
    printf("\n");
    // the same lengths as a fixed length, when they are all equal
    bool equal = !lens.empty();
    for (uint32_t l : lens) equal = equal && l == lens[0];
    if (equal) {
        std::vector<uint64_t> c2(parts + 1);
        mcrc::shard_cuts(nullptr, lens[0], lens.size(), parts, c2.data());
        CHECK(c2 == cuts);
    }
    return 0;
}

// The route of one batch as a test describes it (no array is read).
int print_route(char **v) {
    crc32c_spans s{};
    s.n = strtoull(v[0], nullptr, 0);
    s.len = (uint32_t)strtoul(v[1], nullptr, 0);
    s.stride = strtoull(v[2], nullptr, 0);
    s.offsets = atoi(v[3]) ? kSomeOffsets : nullptr;
    s.lens = atoi(v[4]) ? kSomeLens : nullptr;
    s.base = (const void *)(0x7f0000000000ull + strtoull(v[5], nullptr, 0));
    s.base_bytes = strtoull(v[6], nullptr, 0);
    static const char *const names[] = {"empty", "invalid", "k1", "small", "k5", "id_blocks", "id_spans",
                                        "id_final", "planned"};
    printf("%s\n", names[(int)mcrc::span_route(s, strtoull(v[7], nullptr, 0))]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "cuts")) return print_cuts(atoi(argv[2]));
    if (argc == 10 && !strcmp(argv[1], "route")) return print_route(argv + 2);
    fixed_length_routes();
    small_rule();
    item_routes();
    geometry();
    pipeline_cuts();
    printf("host_route ok\n");
    return 0;
}
