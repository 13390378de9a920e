// k_walk.h -- the fallback lists' gather and scatter, the iov chain fold and
// the device-side page walk.
#pragma once

#include "k_plan.h"

namespace mcrc_dev {

// Fallback lists: gather the listed items' offsets / scatter their results.
// (route 0, k_census: k_lines took no image, the list is every image: the
// identity)
__global__ void k_gather_offs(const uint64_t *offsets, const uint32_t *idx, const uint32_t *nidx, uint64_t *out,
                              const uint32_t *route) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t nn = *nidx;
    const bool all = route && *route == 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x)
        out[i] = offsets[all ? i : idx[i]];
}
__global__ void k_scatter_ok(const uint8_t *ok_in, const uint32_t *idx, const uint32_t *nidx, uint8_t *ok,
                             const uint32_t *route) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t nn = *nidx;
    const bool all = route && *route == 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x)
        ok[all ? i : idx[i]] = ok_in[i];
}

// Chained CRC over an iov list (the chunked-item read verify of
// storage.c:163-170: crc = crc32c(0, iov0 + 32, ...), then
// crc = crc32c(crc, iov_x) for every chunk).  Given crc_i = crc32c(0, iov_i),
// crc32c(c, B) = crc32c(0, B) ^ M_|B|(c), so chain c folds
//   acc = M_{len_i}(acc) ^ crc_i   over its iovs [first[c], first[c+1]).
// One thread per chain.
__global__ void k_chain(const uint32_t *iov_crc, const uint32_t *lens, uint32_t len, const uint64_t *first,
                        uint64_t nchains, uint32_t *out, const uint32_t *xpow) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c < nchains;
         c += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t acc = 0;
        for (uint64_t i = first[c]; i < first[c + 1]; ++i) {
            const uint32_t l = lens ? lens[i] : len;
            if (acc) acc = mulmodp_dev(acc, xpow8_dev(xpow, l));
            acc ^= iov_crc[i];
        }
        out[c] = acc;
    }
}

// Device-side page walk (storage_compact_readback, storage.c:950-1070): the
// buffer is a sequence of wbuf-sized reads; in each, items are packed from
// offset 0, nkey == 0 ends the wbuf, the next item is at + ITEM_ntotal, and the
// walk stops when fewer than sizeof(item) = 48 bytes remain.  Two passes:
//   k_walk<false>: count the items of wbuf w into cnt[w];
//   (exclusive scan of the counts: prefix[w] = the index of wbuf w's first item)
//   k_walk<true>: walk again and write item prefix[w] + c's offset and, for a
//     planned verify, its plan entries (count_item: what k_count would write
//     after reading the header a second time), so no k_count pass follows.
// Round 4: the count pass also keeps the first kslot offsets of each wbuf
// (out.slots), and the emit pass of a verify that needs offsets only (K5)
// copies them instead of walking a wbuf again (the second walk re-read every
// header line from HBM: 0.15 ms per 300 pages); a wbuf of more than kslot
// items is walked again as before.
// One wave per wbuf.  The walk is a dependent chain, so each round trip
// guesses: lane j reads the header at off + j * s, s = the last item's
// ITEM_ntotal.  Lane j's guess is right iff every lane before it holds an item
// of exactly s bytes; the first lane m where that fails (a ballot) still sits
// on a true item boundary, so lanes [0, m) are items, lane m is one too unless
// it ends the wbuf (nkey == 0, or fewer than 48 bytes left), and the walk goes
// on from lane m's item end with s = its ntotal.  Whatever the data, the
// result is the sequential walk's (tests/test_walk_model.py restates it);
// equal-sized items cost one round trip per 64 of them.  Round 6: after a
// round trip whose guesses broke at lane 0 or 1 the next one guesses once
// (lane 0 alone reads a header), and widens again when that guess holds.

struct WalkOut {
    uint32_t *cnt;           // count pass: items per wbuf
    const uint32_t *prefix;  // emit pass: index of each wbuf's first item (nw + 1 entries)
    uint64_t *offs;          // emit pass: item offsets from base
    uint64_t *nunit;         // emit pass, planned verify (else nullptr): k_count's entries
    uint4 *irec;
    uint8_t *fast;
    unsigned long long *err; // emit pass: wbufs whose two walks disagree (must stay 0)
    uint64_t *slots;         // count pass: the first kslot item offsets of wbuf w at w * kslot
    uint32_t kslot;          // (0: none kept)
};

// a: base, base_bytes (the walked bytes), region (= wbuf), and for the plan
// entries xpow, tab8, span_acc.
template <bool EMIT>
__global__ __launch_bounds__(64 * kWalkWaves) void k_walk(SpanArgs a, uint64_t nw, WalkOut out) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    __shared__ __attribute__((aligned(16))) uint32_t s8[EMIT ? kTab8Dwords : 1];
    Tab8 t8{s8};
    const bool plan = EMIT && out.irec;
    if (plan) t8 = load_tab8(s8, a.tab8);
    const uint32_t j = threadIdx.x & 63u;
    const uint64_t wbuf = a.region;
    // the wave's wbuf index as a scalar: the walk state (off, s, c) is then
    // wave-uniform in the compiler's view too, and the loops are scalar loops
    // (with the index in a VGPR the walk went wrong on large page sets)
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t w = (uint64_t)blockIdx.x * kWalkWaves + wave; w < nw; w += (uint64_t)gridDim.x * kWalkWaves) {
        const uint64_t start = w * wbuf, size = a.base_bytes - start < wbuf ? a.base_bytes - start : wbuf;
        const uint8_t *wb = a.base + start;
        const uint64_t first = EMIT ? out.prefix[w] : 0;
        // the count pass's item count of this wbuf: the emit pass never writes
        // past it (into the next wbuf's slots) and checks that it walks the
        // same number of items (the walk invariant; see DESIGN.md section 3 on
        // the round-2 readlane variants that broke it)
        const uint64_t expect = EMIT ? out.prefix[w + 1] - first : 0;
        if (EMIT && !plan && out.slots && expect <= out.kslot) {  // the count pass kept them all
            for (uint64_t i = j; i < expect; i += 64) out.offs[first + i] = out.slots[w * out.kslot + i];
            continue;
        }
        uint64_t off = 0, s = 0;  // wave-uniform: next item, stride guess (0: none yet)
        uint32_t c = 0;           // items walked so far
        // guesses this round trip: 64, or 1 after a round trip whose guesses
        // broke at once (round 6: a wbuf of mixed sizes breaks every guess at
        // its first lane, and 63 wasted header reads per item flooded HBM --
        // 19 us per round trip on the mixed pages; one read per item until a
        // size repeats)
        uint32_t wid = 1;
        while (off + 48 <= size) {
            const uint64_t o = off + j * s;
            const bool in = j < wid && (j == 0 || s != 0) && o + 48 <= size;  // (s < 2^33: no overflow)
            ItemHdr h{0u, 0u, 0u, 0u};
            if (in) h = parse_hdr(wb + o);
            const uint64_t nt = h.ntotal(a.cfl);
            const bool item = in && h.nkey != 0;
            // m = the first lane whose successor's guess is wrong (wid: none;
            // lanes past wid guessed nothing)
            const uint64_t brk = __ballot(!(item && nt == s)) & (wid >= 64u ? ~0ull : (1ull << wid) - 1ull);
            const uint32_t m = brk ? (uint32_t)__ffsll((unsigned long long)brk) - 1u : wid;
            // lane m (if any) is on a true boundary: an item, or the end of the
            // wbuf.  Its flag and size are read out of lane m into scalars
            // (v_readlane: the walk state is scalar).  Round 6: the walk kept
            // its state in VGPRs through round 5, broadcast with ds_bpermute,
            // because readlane variants had gone wrong on large page sets in
            // round 2 -- the 64-bit shift hazard of the header parse (DESIGN.md
            // 3.6), since removed; the bpermutes' LDS round trips were most of
            // a narrow round trip's time
            const uint32_t src = m < wid ? m : 0u;
            const bool last_item = m < wid && __builtin_amdgcn_readlane((int)item, (int)src) != 0;
            const uint64_t nt_m = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)nt, (int)src) |
                                  ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(nt >> 32), (int)src)
                                   << 32);
            const uint32_t k = m < wid ? m + (last_item ? 1u : 0u) : wid;  // items this round trip
            if (!EMIT && out.slots && j < k && c + j < out.kslot) out.slots[w * out.kslot + c + j] = start + o;
            if (EMIT && j < k && c + j < expect) {
                const uint64_t i = first + c + j;
                out.offs[i] = start + o;
                if (plan) count_item<1>(a, i, item_desc(a, start + o, h, true), t8, out.nunit, out.irec, out.fast);
            }
            c += k;
            if (m == wid) {
                off += wid * s;  // every guess right: the size repeats
                wid = 64u;
            } else if (!last_item) {
                break;  // lane m ends the wbuf
            } else {
                off += m * s + nt_m;
                s = nt_m;
                wid = m <= 1u ? 1u : 64u;
            }
        }
        if (!EMIT && j == 0) out.cnt[w] = c;
        if (EMIT && j == 0 && c != expect) atomicAdd(out.err, 1ull);
    }
}

}  // namespace mcrc_dev
