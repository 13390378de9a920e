// k_scrub.h -- crc32c_scrub_pages: the two list rules a caller of the repair
// flow ran on the host between crc32c_triage_pages and the repair calls, and
// the flip log, as kernels over the merged list where k_recover_merge left it
// (ascending by offset, whole: the scrub sizes its scratch by the list).
//
//   k_scrub_headers  the list for crc32c_repair_headers:
//                    per piece every kind-0 entry, then the piece's walk end --
//                    the end of its last walked entry (kinds 4 and 6 are no
//                    walked entries), or the piece's start when it has none --
//                    when that entry is not kind 0 and 48 bytes of the piece
//                    remain there (over the second list of CRC32C_SCRUB_GAPS a
//                    gap entry is listed as a kind-0 entry is, and the walk
//                    end takes its place in front of the gap starts behind it);
//   k_scrub_items    the list for crc32c_repair_items:
//                    every kind-0 entry with a length, and every suspect that
//                    ends at or before the next proven entry (kind 1 or 4) and
//                    starts at or behind the end of the last suspect kept;
//   k_scrub_log      a repair stage's verdicts compacted into the log, in list
//                    order;
//   k_scrub_log_bytes  the same for a byte stage (CRC32C_SCRUB_BYTES): a
//                    repaired entry's mask becomes one log entry per set bit.
// The two list kernels run twice around a k_scan32, as the walk does: one wave
// per piece, its entries 64 a round.  Both rules are piece-local: a piece's
// entries are one range of the list, a suspect is a sane candidate and so lies
// inside its own piece, hence ends at or before any proven entry of a later
// piece and starts behind any suspect kept in an earlier one.
//
// CRC32C_SCRUB_GAPS (the contract's gap_starts, header_list' and item_list'):
//   k_scrub_gaps          the end of every kind-4 entry that is no entry's
//                         offset and has 48 bytes of its piece behind it, as
//                         entries of a list of their own: the offset and the
//                         ITEM_ntotal of the header there when it is sane,
//                         else 0;
//   k_scrub_gap_merge     the merged list and the gap entries in one second
//                         list, ascending (a gap start is no entry's offset:
//                         no ties), with two kind arrays: a gap entry is
//                         kKindGap for the headers, and for the items
//                         kKindSuspect when it has a length, else kKindGap.
// Both list kernels run over the second list as they do over the triage's own:
// k_scrub_headers by the rule above, and in k_scrub_items a gap entry with a
// length goes through the filter as the suspect its kind says, one without is
// of no kind it takes.
// A gap start lies in its entry's piece, so both rules stay piece-local.
#pragma once

#include "k_recover.h"

namespace mcrc_dev {

constexpr uint32_t kScrubLogThreads = 1024;  // k_scrub_log's round
constexpr uint8_t kKindGap = 7;              // a gap start in the second list (never leaves the device)

// The merged list as the triage left it (n: all of its entries).
struct ScrubList {
    const uint64_t *offs;
    const uint32_t *lens;
    const uint8_t *kind;
    uint64_t n;
};

// The greedy chain of the suspects kept is sequential, but only along the
// suspects that end in time: the wave goes through those in order, as
// k_salvage_pick goes through the verified candidates.  The next proven entry
// behind a lane's own is the first one above it in the round's ballot, or the
// first one of the rounds behind it (`nxt`, looked for once per proven entry:
// the search resumes where it last ended).
//   EMIT false: cnt[w] = the piece's entries of the item list;
//   EMIT true:  entry prefix[w] + r is written to out, when below cap.
template <bool EMIT>
__global__ __launch_bounds__(64 * kWalkWaves) void k_scrub_items(ScrubList l, uint64_t wbuf, uint64_t base_bytes,
                                                                 uint64_t nw, uint32_t *cnt, const uint32_t *prefix,
                                                                 uint64_t *out, uint64_t cap) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t j = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the lanes above this one, by halves (no 64-bit shift by a register amount)
    const uint32_t above_lo = j < 32u ? 0xfffffffeu << j : 0u;
    const uint32_t above_hi = j < 32u ? 0xffffffffu : 0xfffffffeu << (j - 32u);
    for (uint64_t w = (uint64_t)blockIdx.x * kWalkWaves + wave; w < nw; w += (uint64_t)gridDim.x * kWalkWaves) {
        const uint64_t ps = w * wbuf, pe = mcrc::salvage_piece_end(w, wbuf, base_bytes);
        const uint64_t k0 = sv_lower_bound(l.offs, l.n, ps), k1 = sv_lower_bound(l.offs, l.n, pe);
        const uint64_t first = EMIT ? prefix[w] : 0;
        uint64_t kept_end = 0;
        uint64_t nxt_at = k0, nxt = UINT64_MAX;  // the first proven entry at or behind some index <= kk + 64, or k1
        uint32_t listed = 0;
        for (uint64_t kk = k0; kk < k1; kk += 64) {
            const uint64_t i = kk + j;
            const bool in = i < k1;
            const uint64_t o = in ? l.offs[i] : 0;
            const uint32_t len = in ? l.lens[i] : 0u;
            const uint32_t kd = in ? l.kind[i] : 0u;
            const bool sus = in && kd == kKindSuspect;
            if (__ballot(sus) && nxt_at < kk + 64) {
                nxt_at = k1;
                nxt = UINT64_MAX;
                for (uint64_t c = kk + 64; c < k1; c += 64) {
                    const uint64_t ii = c + j;
                    const uint32_t k2 = ii < k1 ? l.kind[ii] : 0u;
                    const unsigned long long m = __ballot(k2 == 1u || k2 == kKindSalvaged);
                    if (m) {
                        nxt_at = c + (uint64_t)(__ffsll(m) - 1);
                        nxt = l.offs[nxt_at];
                        break;
                    }
                }
            }
            const unsigned long long pm = __ballot(in && (kd == 1u || kd == kKindSalvaged));
            const uint32_t plo = (uint32_t)pm & above_lo, phi = (uint32_t)(pm >> 32) & above_hi;
            const int psrc = plo ? __ffs((int)plo) - 1 : phi ? 32 + __ffs((int)phi) - 1 : -1;
            const uint64_t pin = shfl64(o, psrc < 0 ? 0 : psrc);
            const uint64_t next = psrc < 0 ? nxt : pin;
            bool keep = false;
            unsigned long long m = __ballot(sus && o + len <= next);
            while (m) {
                const int src = __ffsll(m) - 1;
                m &= m - 1;
                const uint64_t so = shfl64(o, src);
                if (so >= kept_end) {
                    kept_end = so + (uint32_t)__shfl((int)len, src, 64);
                    keep |= (int)j == src;
                }
            }
            const bool take = keep || (in && kd == 0u && len != 0u);
            const unsigned long long tm = __ballot(take);
            if (EMIT && take) {
                const uint64_t idx = first + listed + wave_rank(tm);
                if (idx < cap) out[idx] = o;
            }
            listed += (uint32_t)__popcll(tm);
        }
        if (!EMIT && j == 0) cnt[w] = listed;
    }
}

// The gap starts of the merged list l (the triage's; a: the page).  One wave
// per piece, its entries 64 a round.  e, the end of a kind-4 entry, is a gap
// start when 48 bytes of the piece remain there and no entry of the piece
// starts at e: a lower bound over the piece's entries, not a look at the next
// one (a walked kind-0 entry can lie inside a salvaged image's bytes).  The
// kind-4 entries of a piece are disjoint and ascend, so their ends do.
//   EMIT false: cnt[w] = the piece's gap starts;
//   EMIT true:  gap start prefix[w] + r is written to g, when below g.cap: its
//               offset, and the ITEM_ntotal of the header at e when that is
//               sane (parse_hdr reads the 16-byte granules of bytes 28..43 of
//               the 48 that remain), else 0.  (g.kind is not written.)
template <bool EMIT>
__global__ __launch_bounds__(64 * kWalkWaves) void k_scrub_gaps(SpanArgs a, ScrubList l, uint64_t nw, uint32_t *cnt,
                                                                const uint32_t *prefix, RecoverOut g) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t j = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t w = (uint64_t)blockIdx.x * kWalkWaves + wave; w < nw; w += (uint64_t)gridDim.x * kWalkWaves) {
        const uint64_t ps = w * a.region, pe = mcrc::salvage_piece_end(w, a.region, a.base_bytes);
        const uint64_t k0 = sv_lower_bound(l.offs, l.n, ps), k1 = sv_lower_bound(l.offs, l.n, pe);
        const uint64_t first = EMIT ? prefix[w] : 0;
        uint32_t listed = 0;
        for (uint64_t kk = k0; kk < k1; kk += 64) {
            const uint64_t i = kk + j;
            const bool in = i < k1;
            const uint64_t e = in ? l.offs[i] + l.lens[i] : 0;
            bool gap = in && l.kind[i] == kKindSalvaged && e > ps && e <= pe && pe - e >= 48;
            if (gap) {
                const uint64_t x = k0 + sv_lower_bound(l.offs + k0, k1 - k0, e);
                gap = !(x < k1 && l.offs[x] == e);
            }
            const unsigned long long gm = __ballot(gap);
            if (EMIT && gap) {
                const uint64_t idx = first + listed + wave_rank(gm);
                if (idx < g.cap) {
                    const ItemHdr h = parse_hdr(a.base + e);
                    g.offsets[idx] = e;
                    g.lens[idx] = sane_ntotal(a, e, h, true);
                }
            }
            listed += (uint32_t)__popcll(gm);
        }
        if (!EMIT && j == 0) cnt[w] = listed;
    }
}

// The second list: l's entries and the ng gap entries (goffs, glens),
// ascending.  An entry's place is its own index plus the other list's entries
// below it.  out.kind is the headers' kind array, ikind the items'.
__global__ __launch_bounds__(256) void k_scrub_gap_merge(ScrubList l, const uint64_t *goffs, const uint32_t *glens,
                                                         uint64_t ng, RecoverOut out, uint8_t *ikind) {
    MCRC_VGPR_FLOOR();
    for (uint64_t t = blockIdx.x * 256ull + threadIdx.x; t < l.n + ng; t += gridDim.x * 256ull) {
        const bool own = t < l.n;
        const uint64_t i = own ? t : t - l.n;
        const uint64_t o = own ? l.offs[i] : goffs[i];
        const uint64_t at = i + (own ? sv_lower_bound(goffs, ng, o) : sv_lower_bound(l.offs, l.n, o));
        if (at >= out.cap) continue;
        const uint32_t len = own ? l.lens[i] : glens[i];
        out.offsets[at] = o;
        out.lens[at] = len;
        out.kind[at] = own ? l.kind[i] : kKindGap;
        ikind[at] = own ? l.kind[i] : len ? kKindSuspect : kKindGap;
    }
}

// The header list, over the triage's list or the second list.  A gap entry
// (kKindGap: the second list only) is listed as a kind-0 entry is and is no
// walked entry.  The walk end lies in front of the gap starts behind it, so it
// is found first, in a pass over the kinds; the listing pass then leaves its
// place free (`below` entries in front of it) and moves the entries behind it
// up by one.  A walk end at which a gap entry stands is listed once, as that
// entry.  (Over a list without gap entries that test never fires, and behind a
// good last walked entry every kind-0 entry of the piece lies in front of the
// walk end: below == listed, the walk end comes last.)
//   EMIT false: cnt[w] = the piece's entries of the header list;
//   EMIT true:  entry prefix[w] + r is written to out, when below cap.
template <bool EMIT>
__global__ __launch_bounds__(64 * kWalkWaves) void k_scrub_headers(ScrubList l, uint64_t wbuf, uint64_t base_bytes,
                                                                        uint64_t nw, uint32_t *cnt,
                                                                        const uint32_t *prefix, uint64_t *out,
                                                                        uint64_t cap) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t j = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t w = (uint64_t)blockIdx.x * kWalkWaves + wave; w < nw; w += (uint64_t)gridDim.x * kWalkWaves) {
        const uint64_t ps = w * wbuf, pe = mcrc::salvage_piece_end(w, wbuf, base_bytes);
        const uint64_t k0 = sv_lower_bound(l.offs, l.n, ps), k1 = sv_lower_bound(l.offs, l.n, pe);
        const uint64_t first = EMIT ? prefix[w] : 0;
        uint64_t end = ps;   // the walk end: behind the last walked entry
        uint32_t last = 1u;  // that entry's kind (none: as a good one)
        for (uint64_t kk = k0; kk < k1; kk += 64) {
            const uint64_t i = kk + j;
            const bool in = i < k1;
            const uint32_t kd = in ? l.kind[i] : (uint32_t)kKindSalvaged;
            const unsigned long long wm = __ballot(in && kd != kKindSalvaged && kd != kKindSuspect && kd != kKindGap);
            if (wm) {
                const int src = 63 - __clzll((long long)wm);
                last = (uint32_t)__shfl((int)kd, src, 64);
                end = shfl64(in ? l.offs[i] + l.lens[i] : 0, src);
            }
        }
        bool take = last != 0u && end >= ps && end <= pe && pe - end >= 48;
        if (take) {
            const uint64_t x = k0 + sv_lower_bound(l.offs + k0, k1 - k0, end);
            take = !(x < k1 && l.offs[x] == end && l.kind[x] == kKindGap);
        }
        uint32_t listed = 0, below = 0;
        for (uint64_t kk = k0; kk < k1; kk += 64) {
            const uint64_t i = kk + j;
            const bool in = i < k1;
            const uint64_t o = in ? l.offs[i] : 0;
            const uint32_t kd = in ? l.kind[i] : (uint32_t)kKindSalvaged;
            const bool zero = in && (kd == 0u || kd == kKindGap);
            const unsigned long long zm = __ballot(zero);
            if (EMIT && zero) {
                const uint64_t idx = first + listed + wave_rank(zm) + (take && o > end ? 1u : 0u);
                if (idx < cap) out[idx] = o;
            }
            listed += (uint32_t)__popcll(zm);
            below += (uint32_t)__popcll(__ballot(zero && o < end));
        }
        if (EMIT) {
            if (take && j == 0 && first + below < cap) out[first + below] = end;
        } else if (j == 0) {
            cnt[w] = listed + (uint32_t)take;
        }
    }
}

// The log of one repair stage: entry i of its list with ok[i] = kItemRepaired
// becomes (list[i], bit[i], by), the r-th such entry at log index at + r when
// that is below cap.  One workgroup, kScrubLogThreads entries a round (a list
// is a few entries per damaged image).
__global__ __launch_bounds__(kScrubLogThreads) void k_scrub_log(const uint64_t *list, const uint8_t *ok,
                                                                const uint64_t *bit, uint64_t n, uint32_t by,
                                                                uint64_t at, uint64_t cap, uint64_t *flip_offsets,
                                                                uint64_t *flip_bits, uint8_t *flip_by) {
    MCRC_VGPR_FLOOR();
    __shared__ uint32_t sh[kScrubLogThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t carry = at;
    for (uint64_t i0 = 0; i0 < n; i0 += kScrubLogThreads) {
        const uint64_t i = i0 + threadIdx.x;
        const bool hit = i < n && ok[i] == kItemRepaired;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) sh[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t k = 0; k < kScrubLogThreads / 64; ++k) {
            before += k < w ? sh[k] : 0u;
            all += sh[k];
        }
        __syncthreads();
        const uint64_t idx = carry + before + wave_rank(m);
        if (hit && idx < cap) {
            flip_offsets[idx] = list[i];
            flip_bits[idx] = bit[i];
            flip_by[idx] = (uint8_t)by;
        }
        carry += all;
    }
}

// The log of a byte stage (CRC32C_SCRUB_BYTES): entry i of its list with
// ok[i] = kItemRepaired, located at image byte byte[i] with mask[i], becomes
// popcount(mask[i]) consecutive log entries (list[i], 8 byte[i] + b, by), one
// per set bit b, ascending.  An entry's first log index is at plus the
// popcounts of the repaired entries in front of it: a wave scan, the waves'
// sums through LDS, and the carry of the rounds before.  Written only below
// cap; *total takes the stage's exact bit count whatever cap is.  One
// workgroup, kScrubLogThreads entries a round, as k_scrub_log.
__global__ __launch_bounds__(kScrubLogThreads) void k_scrub_log_bytes(const uint64_t *list, const uint8_t *ok,
                                                                      const uint64_t *byte, const uint8_t *mask,
                                                                      uint64_t n, uint32_t by, uint64_t at,
                                                                      uint64_t cap, uint64_t *flip_offsets,
                                                                      uint64_t *flip_bits, uint8_t *flip_by,
                                                                      unsigned long long *total) {
    MCRC_VGPR_FLOOR();
    __shared__ uint32_t sh[kScrubLogThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t carry = at;
    for (uint64_t i0 = 0; i0 < n; i0 += kScrubLogThreads) {
        const uint64_t i = i0 + threadIdx.x;
        const bool hit = i < n && ok[i] == kItemRepaired;
        const uint32_t m = hit ? mask[i] : 0u;
        const uint32_t c = (uint32_t)__popc(m);
        const uint32_t incl = wave_incl_scan(c, lane);
        if (lane == 63) sh[w] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t k = 0; k < kScrubLogThreads / 64; ++k) {
            before += k < w ? sh[k] : 0u;
            all += sh[k];
        }
        __syncthreads();
        if (m) {
            uint64_t idx = carry + before + (incl - c);
            const uint64_t o = list[i], k0 = 8 * byte[i];
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b) {
                if (!(m & (1u << b))) continue;
                if (idx < cap) {
                    flip_offsets[idx] = o;
                    flip_bits[idx] = k0 + b;
                    flip_by[idx] = (uint8_t)by;
                }
                ++idx;
            }
        }
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry - at;
}

}  // namespace mcrc_dev
