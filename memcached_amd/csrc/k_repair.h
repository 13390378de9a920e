// k_repair.h -- crc32c_repair_items: the bit a damaged image's stored CRC names.
//
// The images' CRCs come from the item kernels (run_items<2> with SpanArgs::out
// set: the CRC of every sane image into out[], the image left alone).  From
// there, with S = out ^ stored (the rule: include/crc32c_batch.h; the
// arithmetic: repair_geom.h):
//   k_repair_count   a thread per image: the verdicts that need no search
//                    (not sane, too long, intact) and, for an image with
//                    S != 0, a 1 in lcnt[] and its chunks in ccnt[]; the
//                    spans' sum for the work bound;
//   (k_scan32 over both: the listed images' and their chunks' prefixes)
//   k_repair_emit    the listed images' records, ascending, each with its
//                    first chunk;
//   k_repair_search  the hot path: a lane per chunk of kRepairChunk byte
//                    steps, V <- V x^-8 by a 256-entry LDS table, a hit when V
//                    is a single bit inside its top byte;
//   k_repair_apply   a thread per listed image: the located bit accepted or
//                    not, ok[] and bit[] written, the bit inverted by one
//                    plain byte store.
#pragma once

#include "k_plan.h"
#include "k_salvage.h"
#include "repair_geom.h"

namespace mcrc_dev {

constexpr uint8_t kItemRepaired = 5;  // CRC32C_ITEM_REPAIRED

// A listed image: S != 0, L <= max_span.
struct RepairRec {
    uint64_t off;  // the image's offset
    uint32_t len;  // L = ITEM_ntotal - 32
    uint32_t syn;  // S
    uint32_t idx;  // its entry of the caller's list
    uint32_t pad;
};

struct RepairArgs {
    const uint32_t *crc;      // the images' computed CRCs (valid for the sane ones)
    uint32_t max_span;
    uint8_t *ok;              // the caller's verdicts ...
    uint64_t *bit;            // ... and positions
    uint32_t *lcnt, *ccnt;    // per image: listed (0 / 1), its chunks
    // [0] the listed images' spans, [1] bad, [2] repaired
    unsigned long long *ctr;
};
enum { kRpWork = 0, kRpBad = 1, kRpRepaired = 2, kRpWords = 3 };
static_assert(kRpBad == kRpWork + 1 && kRpRepaired == kRpBad + 1, "block_add64 adds to two adjacent words");

// a: base, base_bytes, region, cfl, offsets, n.
__global__ __launch_bounds__(256) void k_repair_count(SpanArgs a, RepairArgs r) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    uint64_t work = 0, bad = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const ItemDesc d = fetch_item<1>(a, i);
        const bool fits = d.sane && d.len <= r.max_span;
        const uint32_t syn = fits ? r.crc[i] ^ d.aux : 0u;
        const bool listed = fits && syn != 0u;
        r.lcnt[i] = listed;
        r.ccnt[i] = listed ? (uint32_t)mcrc::repair_nchunks(d.len) : 0u;
        if (listed) {
            work += d.len;
        } else {
            r.ok[i] = fits;
            r.bit[i] = mcrc::kRepairNoBit;
            bad += !fits;
        }
    }
    block_add64(r.ctr + kRpWork, work, bad, threadIdx.x & 63u);
}

// lpre, cpre: the exclusive scans of lcnt and ccnt.
__global__ __launch_bounds__(256) void k_repair_emit(SpanArgs a, RepairArgs r, const uint32_t *lpre,
                                                     const uint32_t *cpre, RepairRec *recs, uint32_t *first,
                                                     uint32_t *found, uint64_t nl) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        if (!r.lcnt[i]) continue;
        const uint32_t q = lpre[i];
        if (q >= nl) continue;  // (the count the host sized the records by)
        const ItemDesc d = fetch_item<1>(a, i);
        recs[q] = RepairRec{a.offsets[i], d.len, r.crc[i] ^ d.aux, (uint32_t)i, 0u};
        first[q] = cpre[i];
        found[q] = mcrc::kRepairNone;
    }
}

// The search.  Chunk w of all the listed images' chunks belongs to the record q
// with first[q] <= w < first[q + 1] (a binary search: first[] ascends strictly,
// every listed image has a chunk) and is its chunk c = w - first[q]: the byte
// steps j0 = c kRepairChunk .. of V_j = S x^(-8 j).  The chunk's first value is
// one product with a power of x from the table (repair_chunk_pow; none for an
// image's first chunk, which is all a short image has), every further one a
// shift and an LDS lookup.  At most one position of an image hits (the order
// of x), so the lane that finds it stores it with no atomic.
__global__ __launch_bounds__(256) void k_repair_search(const RepairRec *recs, const uint32_t *first, uint64_t nl,
                                                       uint64_t nchunks, const uint32_t *xpow, uint32_t *found) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    __shared__ uint32_t inv8[256];
    if (threadIdx.x < 256) inv8[threadIdx.x] = mcrc::repair_unstep8(threadIdx.x << 24);
    __syncthreads();
    for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < nchunks;
         w += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = nl;  // the last q with first[q] <= w
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (first[mid] <= w) lo = mid;
            else hi = mid;
        }
        const RepairRec rec = recs[lo];
        const uint64_t j0 = (w - first[lo]) * mcrc::kRepairChunk, steps = mcrc::repair_steps(rec.len);
        if (j0 >= steps) continue;
        const uint32_t ns = (uint32_t)min((uint64_t)mcrc::kRepairChunk, steps - j0);
        uint32_t v = rec.syn;
        if (j0) v = mulmodp_dev(v, xpow8_dev(xpow, mcrc::repair_chunk_pow(j0)));
        for (uint32_t j = 0; j < ns; ++j) {
            if (mcrc::repair_hit(v)) found[lo] = (uint32_t)(8u * (j0 + j)) + (uint32_t)__clz((int)v);
            v = (v << 8) ^ inv8[v >> 24];
        }
    }
}

// The verdicts of the listed images.  locate_only: nothing is written into the
// buffer.
__global__ __launch_bounds__(256) void k_repair_apply(SpanArgs a, RepairArgs r, const RepairRec *recs,
                                                      const uint32_t *found, uint64_t nl, uint32_t locate_only) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    uint64_t rep = 0, bad = 0;
    uint8_t *const base = const_cast<uint8_t *>(a.base);
    for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < nl;
         q += (uint64_t)gridDim.x * blockDim.x) {
        const RepairRec rec = recs[q];
        const uint32_t t = found[q];
        bool accept = false;
        uint64_t k = mcrc::kRepairNoBit;
        if (t != mcrc::kRepairNone) {
            k = 224 + mcrc::repair_q_of_t(t, rec.len);
            const uint64_t nt = (uint64_t)rec.len + 32, kb = k / 8;
            const uint8_t m = (uint8_t)(1u << (uint32_t)(k % 8));
            // (not a length bit: nbytes is as the header has it)
            const ItemHdr h = parse_hdr(a.base + rec.off);
            uint8_t c0 = base[rec.off + nt - 2], c1 = base[rec.off + nt - 1];
            if (kb == nt - 2) c0 ^= m;
            if (kb == nt - 1) c1 ^= m;
            accept = !mcrc::repair_length_bit(k) && mcrc::salvage_has_crlf(h.nbytes) && mcrc::salvage_crlf(c0, c1);
            if (accept && !locate_only) base[rec.off + kb] ^= m;
        }
        r.ok[rec.idx] = accept ? kItemRepaired : 0;
        r.bit[rec.idx] = accept ? k : mcrc::kRepairNoBit;
        rep += accept;
        bad += !accept;
    }
    block_add64(r.ctr + kRpBad, bad, rep, threadIdx.x & 63u);
}

}  // namespace mcrc_dev
