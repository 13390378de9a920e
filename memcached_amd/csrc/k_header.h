// k_header.h -- crc32c_repair_headers: the one inverted length bit of an item
// header, found by trying the 42 headers one bit away.
//
// A header bit that decides ITEM_ntotal moves the image's end, so the image no
// longer verifies over its own span and crc32c_repair_items refuses it
// (repair_length_bit).  Each of the 42 headers one such bit away names a span
// of its own; the one whose CRC equals the stored one, with a value that ends
// in CRLF, is the header that was written (the rule: include/crc32c_batch.h;
// the arithmetic: header_geom.h).  Three steps:
//   k_header_variants  a wave per listed header, a lane per variant (lane 42:
//                      the header as it stands): sanity from the fields and
//                      the two CRLF bytes make a candidate; count, then emit
//                      around a k_scan32, as the walk does;
//   (the candidates' CRCs over the buffer as it stands: the span kernels,
//    run_spans over the records' offsets and lengths)
//   k_header_apply     a wave per header: a candidate hits when its CRC, XOR
//                      the x^t of its bit, equals the stored one; exactly one
//                      hit is accepted and the bit inverted by one plain byte
//                      store.
#pragma once

#include "k_plan.h"
#include "k_repair.h"
#include "k_salvage.h"
#include "header_geom.h"

namespace mcrc_dev {

constexpr uint32_t kHdWaves = 4;  // headers per workgroup

// A candidate beside its span (offset o + 32 and length L' in arrays of their
// own: the span kernels take them as they are).
struct HeaderRec {
    uint32_t idx;  // its entry of the caller's list
    uint32_t var;  // the variant: v < 42 inverts header_bit(v), 42 is the header as it stands
};

struct HeaderArgs {
    uint32_t *cnt;       // per header: its candidates ...
    uint32_t *pre;       // ... and their exclusive scan (pre[n]: all of them)
    uint64_t *span_off;  // per candidate, ascending by header and variant
    uint32_t *span_len;
    HeaderRec *recs;
    uint64_t ncap;       // the count the host sized them by
    // [0] the candidate variants' spans (the work bound's sum), [1] the records (the headers that are sane as they
    // stand among them), [2] bad, [3] repaired
    unsigned long long *ctr;
};
enum { kHdWork = 0, kHdCand = 1, kHdBad = 2, kHdRepaired = 3, kHdWords = 4 };
static_assert(kHdCand == kHdWork + 1 && kHdRepaired == kHdBad + 1, "block_add64 adds to two adjacent words");

// (the same test as the walk's: nothing of a header with fewer bytes left is read)
__device__ __forceinline__ bool hd_readable(const SpanArgs &a, uint64_t off) {
    return off < a.base_bytes && a.base_bytes - off >= 48;
}

// a: base, base_bytes, region, cfl, offsets, n.  The header is read once
// (parse_hdr, every lane the same two pieces); lane v applies its bit to the
// fields.
//   EMIT false: cnt[i] = the header's candidates; ctr[kHdWork], ctr[kHdCand] += their totals;
//   EMIT true:  candidate pre[i] + r's record, span offset and length are written.
template <bool EMIT>
__global__ __launch_bounds__(64 * kHdWaves) void k_header_variants(SpanArgs a, HeaderArgs h) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t v = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t work = 0, ncand = 0;  // this lane's share of the wave's headers
    for (uint64_t i = (uint64_t)blockIdx.x * kHdWaves + wave; i < a.n; i += (uint64_t)gridDim.x * kHdWaves) {
        const uint64_t off = a.offsets[i];
        uint32_t nt = 0;  // the candidate's ITEM_ntotal
        if (hd_readable(a, off)) {  // (every lane alike)
            const ItemHdr hd = parse_hdr(a.base + off);
            const uint64_t room = mcrc::header_room(off, a.base_bytes, a.region);
            if (v < mcrc::kHeaderVariants) {
                const mcrc::SalvageHdr f = mcrc::header_variant({hd.nbytes, hd.flags, hd.nkey}, v);
                nt = mcrc::salvage_span(f, a.cfl, room);
                // only a sane variant's last two bytes are fetched: they lie inside the buffer
                if (nt && v != mcrc::kHeaderAsIs &&
                    !(mcrc::salvage_has_crlf(f.nbytes) && mcrc::salvage_crlf(a.base[off + nt - 2], a.base[off + nt - 1])))
                    nt = 0;
            }
        }
        const unsigned long long m = __ballot(nt != 0);
        if (!EMIT) {
            if (v == 0) h.cnt[i] = (uint32_t)__popcll(m);
            // (the header as it stands is what crc32c_verify_items would read of this list: not in the bound)
            work += nt && v != mcrc::kHeaderAsIs ? nt - 32u : 0u;
            ncand += nt != 0;
            continue;
        }
        const uint64_t q = (uint64_t)h.pre[i] +
                           __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (nt && q < h.ncap) {
            h.span_off[q] = off + 32;
            h.span_len[q] = nt - 32u;
            h.recs[q] = HeaderRec{(uint32_t)i, v};
        }
    }
    if constexpr (!EMIT) block_add64(h.ctr + kHdWork, work, ncand, v);  // (kHdCand = kHdWork + 1)
}

// The verdicts.  crc: the candidates' CRCs over the buffer as it stands.
// Inverting bit k of a span of L' bytes changes its CRC by exactly x^t, t =
// header_t(v, L'): x^(8 (t / 8)) from the power table and t % 8 single steps.
// locate_only: nothing is written into the buffer.
__global__ __launch_bounds__(64 * kHdWaves) void k_header_apply(SpanArgs a, HeaderArgs h, const uint32_t *crc,
                                                                uint8_t *ok, uint64_t *bit, uint32_t *lens,
                                                                uint32_t locate_only) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t j = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *const base = const_cast<uint8_t *>(a.base);
    uint64_t bad = 0, rep = 0;  // (lane 0 counts for its wave)
    for (uint64_t i = (uint64_t)blockIdx.x * kHdWaves + wave; i < a.n; i += (uint64_t)gridDim.x * kHdWaves) {
        const uint64_t off = a.offsets[i];
        const uint32_t p0 = h.pre[i];
        const uint32_t cnt = hd_readable(a, off) ? h.pre[i + 1] - p0 : 0u;  // (a header not read has none)
        bool hit = false, asis = false;
        uint32_t var = 0, len = 0;
        if (j < cnt && (uint64_t)p0 + j < h.ncap) {
            const uint32_t e = parse_hdr(a.base + off).exptime;
            const uint64_t q = (uint64_t)p0 + j;
            var = h.recs[q].var;
            len = h.span_len[q];
            if (var == mcrc::kHeaderAsIs) {
                asis = crc[q] == e;
            } else if (var < mcrc::kHeaderBits) {
                const uint64_t t = mcrc::header_t(var, len);
                uint32_t x = xpow8_dev(a.xpow, t >> 3);
                for (uint32_t r = (uint32_t)t & 7u; r; --r) x = mcrc::repair_step(x);
                hit = (crc[q] ^ x) == e;
            }
        }
        const bool intact = __ballot(asis) != 0;
        const bool one = !intact && __popcll(__ballot(hit)) == 1;
        if (intact ? asis : one ? hit : j == 0) {  // one lane writes the verdict
            const uint32_t k = mcrc::header_bit(var);
            if (one && !locate_only) base[off + k / 8] ^= (uint8_t)(1u << (k % 8));
            ok[i] = intact ? 1 : one ? kItemRepaired : 0;
            bit[i] = one ? (uint64_t)k : mcrc::kRepairNoBit;
            lens[i] = intact || one ? len + 32u : 0u;
        }
        if (j == 0) {
            rep += one;
            bad += !intact && !one;
        }
    }
    block_add64(h.ctr + kHdBad, bad, rep, j);  // (kHdRepaired = kHdBad + 1)
}

}  // namespace mcrc_dev
