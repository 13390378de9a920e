// host_route.h -- every decision of the host shim that needs no GPU: where a
// batch goes (span_route, item_route, ptr_route), the launch geometry, the host
// pipeline's order and chunk cuts, a pointer batch's pack plan, the registry of
// page-locked ranges, the shard cuts.  Plain C++ over k_consts.h;
// tests/integration/host_route_check.cpp and ptr_pack_check.cpp run it on the CPU.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "../../include/crc32c_batch.h"
#include "k_consts.h"

namespace mcrc {
namespace dev = mcrc_dev;

// Batches of at most small_max spans (crc32c_set_small_max) take the
// single-launch k_small when their spans are bounded: a group reads its whole
// span alone, so a few multi-MiB spans are left to the planned path.
constexpr uint64_t kSmallSpanMax = 1 << 20;     // fixed-length batches: spans up to 1 MiB
constexpr uint64_t kSmallBaseMax = 8ull << 20;  // else: a buffer of at most 8 MiB (a wbuf, an IO batch)
constexpr uint64_t kCountMax = 0xffffffffull;   // K5 and the plan index spans in 32 bits
constexpr uint64_t kItemsK5Min = 4096;          // item batches from here on: k_census decides on the device

// Every span of `len` bytes is one whole block at its G1 (k_common.h
// one_block) at every alignment mod 128: the batch can go to k_blocks.
static inline bool one_block_len(uint32_t len) {
    for (uint32_t al = 0; al < dev::kGridAlign; ++al) {
        const uint32_t kh = al & 15u;
        const uint32_t vlen = len + ((0u - al - len) & (dev::kGridAlign - 1)), x = vlen + kh;
        const uint32_t g1o = x - dev::kBlockBytes * ((x - 1) / dev::kBlockBytes) - kh;
        const bool drop = dev::frag_drop(len, g1o, vlen);
        if (!(drop ? vlen - g1o == dev::kBlockBytes : len && x == dev::kBlockBytes)) return false;
    }
    return true;
}

// Every span of `len` bytes has K5's fused shape at every alignment (31 or 32
// whole lines after a 4..131-B head): K5 takes the batch whole (config 2r).
static inline bool fused_len(uint32_t len) {
    constexpr uint32_t L = dev::kLineBytes;
    for (uint32_t al = 0; al < L; ++al) {
        const int64_t A = (al + 4 + L - 1) / L * L, B = (al + (int64_t)len) / L * L;
        if (len < 4 || !dev::lines_fused(B - A)) return false;
    }
    return true;
}

// K1's batch shape: equal 4 KiB spans at a 16-B aligned base and stride (the
// lane offset within a step, item * stride, is 32-bit in K1).
static inline bool k1_shape(const crc32c_spans &s) {
    return !s.offsets && !s.lens && s.len == dev::kK1Bytes && ((uintptr_t)s.base & 15u) == 0 &&
           (s.stride & 15u) == 0 && s.stride < (1ull << 31);
}

// Equal spans at a fixed stride must fit the buffer (the kernels read them
// unchecked); spans given by offsets or lengths are checked on the device.
static inline bool fixed_spans_fit(const crc32c_spans &s) {
    if (!s.lens && s.len > dev::kMaxSpan) return false;
    if (s.offsets || s.lens) return true;
    if (s.len > s.base_bytes) return false;
    if (s.n <= 1 || s.stride == 0) return true;
    return (s.n - 1) <= (s.base_bytes - s.len) / s.stride;
}

// Where a span batch goes, in the order tested.  invalid: CRC32C_EINVAL; the
// id_* routes are fixed-length batches that need no plan: k_blocks, k_spans or
// neither (every span its thread's) in front of k_final.
enum class SpanRoute { empty, invalid, k1, small, k5, id_blocks, id_spans, id_final, planned };
static inline SpanRoute span_route(const crc32c_spans &s, uint64_t small_max) {
    if (s.n == 0) return SpanRoute::empty;
    if (!fixed_spans_fit(s)) return SpanRoute::invalid;
    if (k1_shape(s)) return SpanRoute::k1;
    if (s.n <= small_max && (s.lens ? s.base_bytes <= kSmallBaseMax : s.len <= kSmallSpanMax)) return SpanRoute::small;
    if (s.lens || s.len > dev::kSegBytes) return s.n >= kCountMax ? SpanRoute::invalid : SpanRoute::planned;
    if (fused_len(s.len) && s.n < kCountMax) return SpanRoute::k5;
    if (s.len + dev::kGridAlign - 1 <= dev::kWholeMax) return SpanRoute::id_final;
    return one_block_len(s.len) ? SpanRoute::id_blocks : SpanRoute::id_spans;
}

// Where n item images in a buffer of base_bytes go.  k5_ok: they can be
// stamped where they lie (K5's k_fix writes into them; staged host images
// take the planned path).
enum class ItemRoute { small, k5, planned, invalid };
static inline ItemRoute item_route(uint64_t n, uint64_t base_bytes, uint64_t small_max, bool k5_ok = true) {
    if (n <= small_max && base_bytes <= kSmallBaseMax) return ItemRoute::small;
    if (n >= kCountMax) return ItemRoute::invalid;
    return n >= kItemsK5Min && k5_ok ? ItemRoute::k5 : ItemRoute::planned;
}

// One span per 32-lane group of a 1024-thread workgroup, a workgroup per CU
// at most (K1, K5, k_blocks and the unplanned k_spans).
static inline int grid_for(int cus, uint64_t n) {
    return (int)std::max<uint64_t>(1, std::min<uint64_t>((n + 31) / 32, (uint64_t)cus));
}
// k_small's and k_copy's spans per workgroup: enough workgroups to reach every
// CU, at least 8 so that each one's table copy stays a few round trips (2-32
// measured).  (0 CUs count as 1, as k_copy's launch had it;
// k_small's divided n + cus - 1 by max(cus, 1): the same for every cus >= 1.)
static inline uint64_t small_per(int cus, uint64_t n) {
    const uint64_t c = (uint64_t)std::max(cus, 1);
    return std::min<uint64_t>(32, std::max<uint64_t>(8, ((n + c - 1) / c + 1) & ~1ull));
}
// K5: runs of 2 nsr consecutive images per wave, nsr up to kEpoch, enough
// runs for every wave of the grid.
static inline uint32_t k5_nsr(int grid, uint64_t n) {
    const uint64_t waves = (uint64_t)grid * (1024 / 64);
    return (uint32_t)std::min<uint64_t>(dev::kEpoch, std::max<uint64_t>(1, (n + 2 * waves - 1) / (2 * waves)));
}
// One thread per span, 256 per workgroup.  k_final: 1024 workgroups (one
// same-address atomic each: 4096 cost 30 us per 4.8 M items); k_count: 2048
// (profiles/r05_ablations/k_count_grid_ab.txt).
static inline int count_grid(uint64_t n) { return (int)std::min<uint64_t>((n + 255) / 256, 2048); }
static inline int final_grid(uint64_t n) { return (int)std::min<uint64_t>((n + 255) / 256, 1024); }
static inline uint64_t plan_tiles(uint64_t n) { return (n + dev::kPlanTile - 1) / dev::kPlanTile; }
static inline int plan_tile_grid(uint64_t n) { return (int)std::min<uint64_t>(plan_tiles(n), 4096); }
// Planned batches split their blocks evenly over the span kernel's 32-lane
// groups (profiles/r03_ablations/k2_balanced_plan_ab.jsonl), in rounds of
// about 8 GiB of the buffer, 16 at most (profiles/r05_ablations/
// plan_rounds_ab.txt: smaller rounds' restarts cost what their locality gains).
static inline uint32_t span_groups(int cus) { return (uint32_t)cus * (dev::kSpanBlock / 32); }
constexpr uint64_t kRoundBytes = 8ull << 30;
constexpr uint32_t kMaxRounds = 16;
static inline uint32_t plan_rounds(uint64_t base_bytes) {
    const uint64_t rounds = (base_bytes + kRoundBytes - 1) / kRoundBytes;
    return (uint32_t)std::min<uint64_t>(kMaxRounds, std::max<uint64_t>(1, rounds));
}
// Unit capacity of a planned batch: units fit whenever the spans do not
// overlap; overlapping long spans past it are processed whole.
static inline uint64_t plan_cap(uint64_t n, uint64_t base_bytes) {
    return std::min<uint64_t>(n + base_bytes / dev::kSegBytes + 1 + n / 4096, 0xfffffff0ull);
}
// The page walk: a wave per wbuf, kWalkWaves per workgroup.  The count pass
// keeps each wbuf's first offsets, one per 2 KiB (0.4 % of the walked bytes),
// for the emit pass to copy; wbufs under 16 KiB keep none (walked twice).
static inline int walk_grid(uint64_t nw) {
    return (int)std::min<uint64_t>((nw + dev::kWalkWaves - 1) / dev::kWalkWaves, 65535);
}
static inline uint32_t walk_kslot(uint64_t wbuf_bytes) {
    const uint32_t k = (uint32_t)std::min<uint64_t>(wbuf_bytes / 2048, 8192);
    return k < 8 ? 0 : k;
}

static inline uint64_t span_off(const crc32c_spans &s, uint64_t i) { return s.offsets ? s.offsets[i] : i * s.stride; }
static inline uint64_t span_len(const crc32c_spans &s, uint64_t i) { return s.lens ? s.lens[i] : s.len; }

constexpr uint64_t kSlotBytes = 256ull << 20;  // bytes of span data per pipeline stage
constexpr uint64_t kSlotItems = 1ull << 20;

// Host spans must lie in [base, base + base_bytes) and fit a pipeline slot.
static inline bool host_spans_ok(const crc32c_spans &s, uint64_t slot_bytes = kSlotBytes) {
    for (uint64_t i = 0; i < s.n; ++i) {
        const uint64_t off = span_off(s, i), len = span_len(s, i);
        if (off > s.base_bytes || len > s.base_bytes - off || len > slot_bytes - 16) return false;
    }
    return true;
}

// The host pipeline's staging order, by offset: position -> caller index, a
// stable permutation when the caller's order is not sorted; empty: the identity.
static inline std::vector<uint64_t> staging_order(const crc32c_spans &s) {
    std::vector<uint64_t> order;
    for (uint64_t i = 1; i < s.n; ++i)
        if (span_off(s, i) < span_off(s, i - 1)) {
            order.resize(s.n);
            for (uint64_t k = 0; k < s.n; ++k) order[k] = k;
            std::stable_sort(order.begin(), order.end(),
                             [&](uint64_t x, uint64_t y) { return span_off(s, x) < span_off(s, y); });
            break;
        }
    return order;
}

// The pipeline's next chunk: staging positions [k0, k1), their bytes [lo, hi)
// (lo 16-B aligned), at most slot_items spans and slot_bytes bytes.
struct Chunk {
    uint64_t k1, lo, hi;
};
static inline Chunk next_chunk(const crc32c_spans &s, const std::vector<uint64_t> &order, uint64_t k0,
                               uint64_t slot_bytes = kSlotBytes, uint64_t slot_items = kSlotItems) {
    auto idx = [&](uint64_t k) { return order.empty() ? k : order[k]; };
    const uint64_t lo = span_off(s, idx(k0)) & ~15ull;
    uint64_t k1 = k0, hi = lo;
    while (k1 < s.n && k1 - k0 < slot_items) {
        const uint64_t e = span_off(s, idx(k1)) + span_len(s, idx(k1));
        if (std::max(hi, e) - lo > slot_bytes) break;
        hi = std::max(hi, e);
        ++k1;
    }
    return {k1, lo, hi};
}

// Pointer batches (crc32c_ptr_batch): spans with no common base.
static inline uint64_t ptr_len(const crc32c_ptr_batch &b, uint64_t i) { return b.lens ? b.lens[i] : b.len; }

// Where a pointer batch goes.  small: one k_small launch over the spans where
// they lie (a host batch: through the queue, when its spans are short enough
// for it); spans: a host batch is packed into the pipeline's slots, a device
// batch runs as the offsets batch its rebase makes (span_route without the
// small rule).  Small is span_route's rule with the sum of the lengths in
// place of base_bytes: what a group reads is bounded by it, however far apart
// the buffers lie.  sum_len: the lengths' sum (with lens); visible: every span
// is device-visible (a device batch: true).
enum class PtrRoute { empty, invalid, small, spans };
static inline PtrRoute ptr_route(uint64_t n, bool has_lens, uint32_t len, uint64_t sum_len, bool visible,
                                 uint64_t small_max) {
    if (n == 0) return PtrRoute::empty;
    if (!has_lens && len > dev::kMaxSpan) return PtrRoute::invalid;
    if (!visible) return PtrRoute::spans;
    if (n <= small_max && (has_lens ? sum_len <= kSmallBaseMax : len <= kSmallSpanMax)) return PtrRoute::small;
    return n >= kCountMax ? PtrRoute::invalid : PtrRoute::spans;
}
// The span route of a rebased device pointer batch s (offsets given: never K1).
static inline SpanRoute ptr_span_route(const crc32c_spans &s, uint64_t sum_len, uint64_t small_max) {
    switch (ptr_route(s.n, s.lens != nullptr, s.len, sum_len, true, small_max)) {
        case PtrRoute::empty: return SpanRoute::empty;
        case PtrRoute::invalid: return SpanRoute::invalid;
        case PtrRoute::small: return SpanRoute::small;
        default: return span_route(s, 0);
    }
}

// A host pointer batch can be staged: no NULL span that has bytes, none longer
// than a pipeline slot takes.
static inline bool ptr_spans_ok(const crc32c_ptr_batch &b, uint64_t slot_bytes = kSlotBytes) {
    for (uint64_t i = 0; i < b.n; ++i) {
        const uint64_t len = ptr_len(b, i);
        if ((len && !b.ptrs[i]) || len > slot_bytes - 16) return false;
    }
    return true;
}

// The pack plan: the next chunk of a packed pointer batch, spans [k0, k1) in
// caller order (chains fold in it), pos[k - k0] the slot position of span k.
// A span keeps its address mod 16, so the kernels meet the piece splits they
// would meet in place, and owns every 16-byte granule its bytes touch: the
// next span starts on the granule behind them.  A span of no bytes takes no
// room.  The chunk ends before the span that would pass slot_bytes (a multiple
// of 16) or slot_items; bytes: the slot's bytes in use (a multiple of 16).
struct PackChunk {
    uint64_t k1, bytes;
};
static inline PackChunk pack_chunk(const crc32c_ptr_batch &b, uint64_t k0, uint64_t *pos,
                                   uint64_t slot_bytes = kSlotBytes, uint64_t slot_items = kSlotItems) {
    uint64_t k1 = k0, cur = 0;
    for (; k1 < b.n && k1 - k0 < slot_items; ++k1) {
        const uint64_t len = ptr_len(b, k1), at = len ? cur + ((uintptr_t)b.ptrs[k1] & 15u) : cur;
        const uint64_t end = len ? (at + len + 15) & ~15ull : cur;
        if (end > slot_bytes) break;
        pos[k1 - k0] = at;
        cur = end;
    }
    return {k1, cur};
}
// The chunk's bytes copied into its slot: the spans' own bytes and no others.
static inline void pack_copy(const crc32c_ptr_batch &b, uint64_t k0, uint64_t k1, const uint64_t *pos, uint8_t *slot) {
    for (uint64_t k = k0; k < k1; ++k)
        if (const uint64_t len = ptr_len(b, k)) memcpy(slot + pos[k - k0], b.ptrs[k], len);
}

// The page-locked host ranges the library knows (crc32c_host_alloc,
// crc32c_host_register), by first address, each with the device address of its
// first byte: a host span's device view is one O(log R) lookup under a shared
// lock, where the runtime's own answer costs two calls.
class PinRegistry {
  public:
    void record(const void *p, uint64_t bytes, const void *dv) {
        std::unique_lock<std::shared_mutex> lk(mu_);
        ranges_[(uintptr_t)p] = Range{(uintptr_t)p + bytes, (const uint8_t *)dv};
    }
    void forget(const void *p) {
        std::unique_lock<std::shared_mutex> lk(mu_);
        ranges_.erase((uintptr_t)p);
    }
    // The span [p, p + len): inside one recorded range (*dv: its device
    // view), unknown (it starts in none: the runtime may still know it), or
    // cut (it starts in one and runs past its end: no kernel may read it).
    enum class Hit { inside, unknown, cut };
    Hit view(const void *p, uint64_t len, const uint8_t **dv) const {
        const uintptr_t a = (uintptr_t)p;
        std::shared_lock<std::shared_mutex> lk(mu_);
        auto it = ranges_.upper_bound(a);
        if (it == ranges_.begin()) return Hit::unknown;
        --it;
        if (a >= it->second.end) return Hit::unknown;
        if (len > it->second.end - a) return Hit::cut;
        *dv = it->second.dv + (a - it->first);
        return Hit::inside;
    }

  private:
    struct Range {
        uintptr_t end;      // one past the range's last host byte
        const uint8_t *dv;  // the device view of its first byte
    };
    mutable std::shared_mutex mu_;
    std::map<uintptr_t, Range> ranges_;
};

// A host chain fold's staging buffer: the n iovs' CRCs, their lengths, at
// chain_first_off (8-B aligned) the chains' first indices, then the folded CRCs.
static inline uint64_t chain_first_off(uint64_t n) { return (n * 8 + 7) & ~7ull; }
static inline uint64_t chain_stage_bytes(uint64_t n, uint64_t nchains) {
    return n * 8 + (nchains + 1) * 8 + nchains * 4 + 64;
}

// crc32c_shard_cuts (crc32c_batch.h).
static inline void shard_cuts(const uint32_t *lens, uint32_t len, uint64_t n, int parts, uint64_t *cuts) {
    unsigned __int128 total = 0, acc = 0;
    for (uint64_t i = 0; i < n; ++i) total += lens ? lens[i] : len;
    cuts[0] = 0;
    uint64_t i = 0;
    for (int g = 1; g < parts; ++g) {
        const unsigned __int128 target = total * (unsigned)g / (unsigned)parts;
        for (; i < n && acc < target; ++i) acc += lens ? lens[i] : len;
        cuts[g] = i;
    }
    cuts[parts] = n;
}

static inline bool ranges_overlap(const void *p, uint64_t pn, const void *q, uint64_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return pn && qn && a < b + qn && b < a + pn;
}

}  // namespace mcrc
