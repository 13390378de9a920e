// ptr_pack_check.cpp -- the host decisions of the pointer batches
// (memcached_amd/csrc/host_route.h: ptr_route, ptr_span_route, ptr_spans_ok,
// pack_chunk, pack_copy, PinRegistry) run on the CPU.  Every source span of a pack plan is
// its own malloc of exactly the bytes in front of it and its own: a read past
// a span's end is an AddressSanitizer report.
//
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I memcached_amd/csrc ptr_pack_check.cpp
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "host_route.h"

namespace {

using mcrc::PtrRoute;
using mcrc::SpanRoute;

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            exit(1);                                                   \
        }                                                              \
    } while (0)

constexpr uint64_t kSmallMax = mcrc_dev::kSmallMax;

void routes() {
    // no spans, and a fixed length no kernel takes
    CHECK(mcrc::ptr_route(0, false, 100, 0, true, kSmallMax) == PtrRoute::empty);
    CHECK(mcrc::ptr_route(5, false, mcrc_dev::kMaxSpan, 0, true, kSmallMax) == PtrRoute::spans);
    CHECK(mcrc::ptr_route(5, false, mcrc_dev::kMaxSpan + 1, 0, true, kSmallMax) == PtrRoute::invalid);
    // small_max and one more span, by both rules
    for (const uint64_t sm : {(uint64_t)1, (uint64_t)64, kSmallMax}) {
        CHECK(mcrc::ptr_route(sm, false, 4133, 0, true, sm) == PtrRoute::small);
        CHECK(mcrc::ptr_route(sm + 1, false, 4133, 0, true, sm) == PtrRoute::spans);
        CHECK(mcrc::ptr_route(sm, true, 0, 100 * sm, true, sm) == PtrRoute::small);
        CHECK(mcrc::ptr_route(sm + 1, true, 0, 100 * sm, true, sm) == PtrRoute::spans);
    }
    CHECK(mcrc::ptr_route(1, false, 16, 0, true, 0) == PtrRoute::spans);  // (crc32c_set_small_max(0))
    // the lengths' sum at kSmallBaseMax and one byte more: the sum decides, not
    // the distance between the buffers (the rule never sees an address)
    CHECK(mcrc::ptr_route(64, true, 0, mcrc::kSmallBaseMax, true, kSmallMax) == PtrRoute::small);
    CHECK(mcrc::ptr_route(64, true, 0, mcrc::kSmallBaseMax + 1, true, kSmallMax) == PtrRoute::spans);
    // (with lens the fixed len is a decoy, without them the sum is)
    CHECK(mcrc::ptr_route(64, true, 0x7fffffffu, 100, true, kSmallMax) == PtrRoute::small);
    CHECK(mcrc::ptr_route(64, false, 100, ~0ull, true, kSmallMax) == PtrRoute::small);
    // a fixed len at kSmallSpanMax and one more
    CHECK(mcrc::ptr_route(64, false, (uint32_t)mcrc::kSmallSpanMax, 0, true, kSmallMax) == PtrRoute::small);
    CHECK(mcrc::ptr_route(64, false, (uint32_t)mcrc::kSmallSpanMax + 1, 0, true, kSmallMax) == PtrRoute::spans);
    // one span that is not device-visible: packed, however small
    CHECK(mcrc::ptr_route(1, false, 16, 0, false, kSmallMax) == PtrRoute::spans);
    CHECK(mcrc::ptr_route(64, true, 0, 64 * 4133, false, kSmallMax) == PtrRoute::spans);
    // more spans than the kernels index
    CHECK(mcrc::ptr_route(mcrc::kCountMax - 1, true, 0, 1, true, kSmallMax) == PtrRoute::spans);
    CHECK(mcrc::ptr_route(mcrc::kCountMax, true, 0, 1, true, kSmallMax) == PtrRoute::invalid);

    // a rebased device batch: small by the sum, else span_route's answer without its small rule
    crc32c_spans s{};
    s.base = (const void *)0x7f0000000000ull;
    s.base_bytes = 40ull << 30;  // two allocations far apart
    s.offsets = (const uint64_t *)0x1000;
    s.lens = (const uint32_t *)0x2000;
    s.n = 48;
    CHECK(mcrc::span_route(s, kSmallMax) == SpanRoute::planned);  // (what base_bytes would have decided)
    CHECK(mcrc::ptr_span_route(s, 48 * 4133, kSmallMax) == SpanRoute::small);
    CHECK(mcrc::ptr_span_route(s, mcrc::kSmallBaseMax + 1, kSmallMax) == SpanRoute::planned);
    CHECK(mcrc::ptr_span_route(s, 48 * 4133, 0) == SpanRoute::planned);
    s.lens = nullptr;
    const struct {
        uint32_t len;
        SpanRoute route;
    } fixed[] = {{4133, SpanRoute::k5}, {4090, SpanRoute::id_blocks}, {9000, SpanRoute::id_spans},
                 {100, SpanRoute::id_final}, {131073, SpanRoute::planned}};
    for (const auto &f : fixed) {
        s.len = f.len;
        CHECK(mcrc::ptr_span_route(s, 0, 0) == f.route);
        CHECK(mcrc::ptr_span_route(s, 0, kSmallMax) == SpanRoute::small);
    }
    s.n = 0;
    CHECK(mcrc::ptr_span_route(s, 0, kSmallMax) == SpanRoute::empty);
}

// Source spans, each in a malloc of its own that ends with the span's last
// byte; the span starts `phase` bytes into it (malloc returns 16-byte aligned
// blocks, so that is its address mod 16).
struct Sources {
    std::vector<std::unique_ptr<uint8_t, decltype(&free)>> blocks;
    std::vector<const void *> ptrs;
    std::vector<uint32_t> lens;
    void add(uint32_t phase, uint32_t len, bool null = false) {
        uint8_t *p = (uint8_t *)malloc(phase + len ? phase + len : 1);
        CHECK(p && ((uintptr_t)p & 15u) == 0);
        for (uint32_t i = 0; i < phase + len; ++i) p[i] = (uint8_t)(blocks.size() * 37 + i * 11 + 1);
        blocks.emplace_back(p, &free);
        ptrs.push_back(null ? nullptr : p + phase);
        lens.push_back(len);
    }
    crc32c_ptr_batch batch() const {
        crc32c_ptr_batch b{};
        b.ptrs = ptrs.data();
        b.lens = lens.data();
        b.n = ptrs.size();
        return b;
    }
};

// Every chunk of the plan over slots of slot_bytes and slot_items: the
// properties of each, and the packed bytes over both pre-fills.  Returns the
// number of chunks.
uint64_t run_plan(const crc32c_ptr_batch &b, uint64_t slot_bytes, uint64_t slot_items) {
    CHECK(mcrc::ptr_spans_ok(b, slot_bytes));
    std::vector<uint64_t> pos(slot_items);
    uint64_t k0 = 0, chunks = 0;
    while (k0 < b.n) {
        const mcrc::PackChunk ch = mcrc::pack_chunk(b, k0, pos.data(), slot_bytes, slot_items);
        CHECK(ch.k1 > k0 && ch.k1 <= b.n && ch.k1 - k0 <= slot_items);
        CHECK(ch.bytes <= slot_bytes && ch.bytes % 16 == 0);
        uint64_t prev_end = 0;  // positions follow caller order, granules disjoint
        for (uint64_t k = k0; k < ch.k1; ++k) {
            const uint64_t len = mcrc::ptr_len(b, k), at = pos[k - k0];
            if (!len) {
                CHECK(at <= ch.bytes);
                continue;
            }
            CHECK((at & 15u) == ((uintptr_t)b.ptrs[k] & 15u));  // the phase is kept
            const uint64_t g0 = at & ~15ull, g1 = (at + len + 15) & ~15ull;
            CHECK(g0 >= prev_end && g1 <= ch.bytes);  // every granule touched lies inside the slot, after the last span's
            prev_end = g1;
        }
        CHECK(prev_end == ch.bytes);  // no room wasted behind the last span
        // the cut is the earliest allowed: the next span would pass a limit
        if (ch.k1 < b.n && ch.k1 - k0 < slot_items) {
            const uint64_t len = mcrc::ptr_len(b, ch.k1);
            CHECK(len && ((ch.bytes + ((uintptr_t)b.ptrs[ch.k1] & 15u) + len + 15) & ~15ull) > slot_bytes);
        }
        // exact-size slots: a write outside [0, bytes) is a report too
        std::vector<uint8_t> zero(ch.bytes, 0x00), a5(ch.bytes, 0xA5);
        mcrc::pack_copy(b, k0, ch.k1, pos.data(), zero.data());
        mcrc::pack_copy(b, k0, ch.k1, pos.data(), a5.data());
        std::vector<uint8_t> span_byte(ch.bytes, 0);
        for (uint64_t k = k0; k < ch.k1; ++k) {
            const uint64_t len = mcrc::ptr_len(b, k), at = pos[k - k0];
            if (!len) continue;
            CHECK(memcmp(zero.data() + at, b.ptrs[k], len) == 0);
            CHECK(memcmp(a5.data() + at, b.ptrs[k], len) == 0);
            memset(span_byte.data() + at, 1, len);
        }
        for (uint64_t i = 0; i < ch.bytes; ++i)  // and only span bytes were written
            if (!span_byte[i]) CHECK(zero[i] == 0x00 && a5[i] == 0xA5);
        k0 = ch.k1;
        ++chunks;
    }
    return chunks;
}

void pack_plans() {
    // every phase with every short length, a NULL empty span among them
    Sources all;
    for (uint32_t phase = 0; phase < 16; ++phase)
        for (const uint32_t len : {0u, 1u, 15u, 16u, 17u}) all.add(phase, len, len == 0 && phase % 2);
    CHECK(run_plan(all.batch(), mcrc::kSlotBytes, mcrc::kSlotItems) == 1);
    // the item limit: 80 spans in slots of 7
    CHECK(run_plan(all.batch(), 1 << 20, 7) == (80 + 6) / 7);
    // the byte limit.  Spans of 18 bytes at phase 15 take three granules (48 B):
    // a 96-byte slot holds two, a 95-byte one is no slot (not a multiple of 16)
    Sources three;
    for (int i = 0; i < 7; ++i) three.add(15, 18);
    CHECK(run_plan(three.batch(), 96, 100) == 4);
    CHECK(run_plan(three.batch(), 144, 100) == 3);
    CHECK(run_plan(three.batch(), 48, 100) == 7);
    // a span that fills a slot to its last granule, and the longest one a slot takes at any phase
    Sources fill;
    fill.add(0, 256 - 16);
    fill.add(15, 256 - 16 - 15);
    fill.add(15, 256 - 16);
    fill.add(3, 1);
    CHECK(run_plan(fill.batch(), 256, 100) == 4);
    // empty spans take no room and never cut a chunk by bytes
    Sources empties;
    empties.add(0, 64);
    for (int i = 0; i < 5; ++i) empties.add(i, 0, i % 2);
    CHECK(run_plan(empties.batch(), 80, 100) == 1);
    // a fixed len (lens == NULL)
    Sources same;
    for (uint32_t phase = 0; phase < 16; ++phase) same.add(phase, 33);
    crc32c_ptr_batch fixed = same.batch();
    fixed.lens = nullptr;
    fixed.len = 33;
    CHECK(run_plan(fixed, 1 << 12, 100) == 1);
    CHECK(run_plan(fixed, 128, 100) >= 8);

    // what a host batch is refused for
    crc32c_ptr_batch b = all.batch();
    CHECK(mcrc::ptr_spans_ok(b));
    std::vector<const void *> ptrs(all.ptrs);
    ptrs[2] = nullptr;  // (phase 0, len 15)
    b.ptrs = ptrs.data();
    CHECK(!mcrc::ptr_spans_ok(b));
    crc32c_ptr_batch one{};
    const void *p = (const void *)0x1000;  // (never read: only its length is judged)
    one.ptrs = &p;
    one.n = 1;
    one.len = (uint32_t)(mcrc::kSlotBytes - 16);
    CHECK(mcrc::ptr_spans_ok(one));
    one.len += 1;
    CHECK(!mcrc::ptr_spans_ok(one));
}

// The registry: a span inside a range, across its end, in the gaps between
// ranges, below the first and above the last; a range forgotten; one recorded
// again at another size.
void registry() {
    using Hit = mcrc::PinRegistry::Hit;
    mcrc::PinRegistry reg;
    const uint8_t *dv = nullptr;
    auto at = [](uintptr_t a) { return (const void *)a; };
    CHECK(reg.view(at(0x5000), 1, &dv) == Hit::unknown);
    reg.record(at(0x4000), 0x1000, at(0x900000));
    reg.record(at(0x8000), 0x2000, at(0xa00000));
    reg.record(at(0x1000), 0x10, at(0xb00000));
    CHECK(reg.view(at(0x4000), 0x1000, &dv) == Hit::inside && dv == at(0x900000));
    CHECK(reg.view(at(0x4fff), 1, &dv) == Hit::inside && dv == at(0x900fff));
    CHECK(reg.view(at(0x4fff), 0, &dv) == Hit::inside);
    CHECK(reg.view(at(0x4fff), 2, &dv) == Hit::cut);
    CHECK(reg.view(at(0x4000), 0x1001, &dv) == Hit::cut);
    CHECK(reg.view(at(0x5000), 1, &dv) == Hit::unknown);  // one past a range's end
    CHECK(reg.view(at(0x3fff), 2, &dv) == Hit::unknown);  // starts in front of one
    CHECK(reg.view(at(0xfff), 1, &dv) == Hit::unknown && reg.view(at(0xa000), 1, &dv) == Hit::unknown);
    CHECK(reg.view(at(0x9abc), 0x544, &dv) == Hit::inside && dv == at(0xa01abc));
    CHECK(reg.view(at(0x100f), 1, &dv) == Hit::inside && dv == at(0xb0000f));
    reg.forget(at(0x4000));
    CHECK(reg.view(at(0x4000), 1, &dv) == Hit::unknown);
    reg.forget(at(0x4000));  // (twice: nothing to do)
    reg.record(at(0x8000), 0x100, at(0xc00000));
    CHECK(reg.view(at(0x8000), 0x100, &dv) == Hit::inside && dv == at(0xc00000));
    CHECK(reg.view(at(0x8000), 0x101, &dv) == Hit::cut && reg.view(at(0x8100), 1, &dv) == Hit::unknown);
}

}  // namespace

int main() {
    routes();
    pack_plans();
    registry();
    printf("ptr_pack ok\n");
    return 0;
}
