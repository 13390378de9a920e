// k_repair_bytes.h -- crc32c_repair_bytes: the byte a damaged image's stored CRC
// names, and its XOR mask.
//
// The pipeline is crc32c_repair_items' (k_repair.h): the CRCs from the item
// kernels, k_repair_count, the two scans and k_repair_emit as they are (the
// caller's byte[] takes the place of bit[]; its mask[] is zeroed beforehand).
// Two kernels differ:
//   k_repair_bytes_search  the same chunks, binary search and LDS table; a hit
//                          when V is non-zero and confined to its top byte,
//                          stored as (step << 8) | mask (steps < 2^18);
//   k_repair_bytes_apply   a thread per listed image: step -> image byte, the
//                          located pair accepted or not, ok[], byte[] and
//                          mask[] written, the byte corrected by one plain
//                          byte store.
#pragma once

#include "k_repair.h"

namespace mcrc_dev {

static_assert(((uint64_t)mcrc::kRepairBytesSpanMax + 4) << 8 < mcrc::kRepairNone, "a step and a mask fit found[]");

// At most one step of an image hits (repair_geom.h: 4 + L <= 190 235), so the
// lane that finds it stores it with no atomic.
__global__ __launch_bounds__(256) void k_repair_bytes_search(const RepairRec *recs, const uint32_t *first,
                                                             uint64_t nl, uint64_t nchunks, const uint32_t *xpow,
                                                             uint32_t *found) {
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
            if (mcrc::repair_byte_hit(v)) found[lo] = (((uint32_t)j0 + j) << 8) | mcrc::repair_byte_mask(v);
            v = (v << 8) ^ inv8[v >> 24];
        }
    }
}

// The verdicts of the listed images.  r.bit: the caller's byte[].  locate_only:
// nothing is written into the buffer.
__global__ __launch_bounds__(256) void k_repair_bytes_apply(SpanArgs a, RepairArgs r, uint8_t *mask,
                                                            const RepairRec *recs, const uint32_t *found, uint64_t nl,
                                                            uint32_t locate_only) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    uint64_t rep = 0, bad = 0;
    uint8_t *const base = const_cast<uint8_t *>(a.base);
    for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < nl;
         q += (uint64_t)gridDim.x * blockDim.x) {
        const RepairRec rec = recs[q];
        const uint32_t f = found[q];
        bool accept = false;
        uint64_t p = mcrc::kRepairNoBit;
        uint8_t m = 0;
        if (f != mcrc::kRepairNone) {
            p = 28 + mcrc::repair_byte_of_step(f >> 8, rec.len);
            m = (uint8_t)(f & 0xffu);
            const uint64_t nt = (uint64_t)rec.len + 32;
            // (no length bit: nbytes is as the header has it)
            const ItemHdr h = parse_hdr(a.base + rec.off);
            uint8_t c0 = base[rec.off + nt - 2], c1 = base[rec.off + nt - 1];
            if (p == nt - 2) c0 ^= m;
            if (p == nt - 1) c1 ^= m;
            accept = !mcrc::repair_length_mask(p, m) && mcrc::salvage_has_crlf(h.nbytes) && mcrc::salvage_crlf(c0, c1);
            if (accept && !locate_only) base[rec.off + p] ^= m;
        }
        r.ok[rec.idx] = accept ? kItemRepaired : 0;
        r.bit[rec.idx] = accept ? p : mcrc::kRepairNoBit;
        mask[rec.idx] = accept ? m : 0;
        rep += accept;
        bad += !accept;
    }
    block_add64(r.ctr + kRpBad, bad, rep, threadIdx.x & 63u);
}

}  // namespace mcrc_dev
