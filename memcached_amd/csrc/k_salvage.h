// k_salvage.h -- crc32c_salvage_pages: the images the page walk never reached.
//
// One flipped bit in a header ends a wbuf's walk (k_walk.h), and every image
// packed behind it goes unseen.  The salvage looks at every byte offset the
// walk's verified images do not cover as a possible image start and keeps the
// ones whose stored CRC proves them (the rule: include/crc32c_batch.h; the
// arithmetic: salvage_geom.h).  Four steps:
//   k_salvage_regions  the eligible ranges from the walk's lists (a wave per
//                      piece; no pass over the bytes), cut into tiles;
//   k_salvage_scan     the hot path: every eligible offset's header fields
//                      from aligned 16-B loads, sane + CRLF = a candidate;
//   (the candidates' CRCs: the item kernels, run_items<1> over the list)
//   k_salvage_pick     per piece, the verified candidates that start at or
//                      after the end of the last one kept; for
//                      crc32c_triage_pages (SUSPECTS) also the failing ones
//                      that the cursor of the rule reaches.
// Regions, scan and pick each run twice around a k_scan32, as the walk does:
// count, scan the counts, emit in ascending order.
// The page calls behind the salvage (k_recover.h, k_scrub.h) are built from
// the same parts: what their per-piece kernels share stands first here
// (wave_rank, sane_ntotal, sv_lower_bound and the wave helpers), and TileRun,
// a piece's tile bookkeeping, serves both regions kernels.
#pragma once

#include "k_plan.h"
#include "salvage_geom.h"

namespace mcrc_dev {

// The kinds the pick gives an entry (the walk's own verdicts are 0, 1, ...)
constexpr uint8_t kKindSalvaged = 4;  // CRC32C_ITEM_SALVAGED
constexpr uint8_t kKindSuspect = 6;   // CRC32C_ITEM_SUSPECT

// A tile: the eligible offsets [lo, hi) of one aligned block, in a piece that
// ends at pe.
struct SalvageTile {
    uint64_t lo, hi, pe;
};

struct SalvageArgs {
    const uint64_t *walked;    // the walk's images (strictly ascending, < base_bytes) ...
    const uint8_t *walked_ok;  // ... and verdicts; an image covers its bytes when its verdict is not 0 and it is sane
    uint64_t nwalked;
    uint64_t nw;               // pieces
    uint32_t ba;               // the base address mod kSalvageTile
    // [0] list entries out of order or range (the kernels behind the check
    // then do nothing), [1] scanned, [2] ncand, [3] work
    unsigned long long *ctr;
    // the count pass of the regions keeps each piece's first kSvSlots ranges
    // (lo, hi at slots[(w * kSvSlots + r) * 2]) and their number nregs[w]
    uint64_t *slots;
    uint32_t *nregs;
};
constexpr uint32_t kSvSlots = 4;
enum { kSvBad = 0, kSvScanned = 1, kSvCand = 2, kSvWork = 3, kSvWords = 4 };
static_assert(kSvWork == kSvCand + 1, "block_add64 adds to two adjacent words");

// Device lists: every entry below base_bytes and above its predecessor.
__global__ void k_salvage_check(SalvageArgs s, uint64_t base_bytes) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    uint32_t nb = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < s.nwalked;
         i += (uint64_t)gridDim.x * blockDim.x)
        nb += s.walked[i] >= base_bytes || (i && s.walked[i - 1] >= s.walked[i]);
    wave_sum(nb);  // (not count_bad: its LDS word would be shared with the kernels that use it)
    if (__lane_id() == 0 && nb) atomicAdd(s.ctr + kSvBad, (unsigned long long)nb);
}

// The first index of a[0, n) whose entry is not below key.
__device__ __forceinline__ uint64_t sv_lower_bound(const uint64_t *a, uint64_t n, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
    return v;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    return (uint64_t)__shfl((unsigned long long)v, src, 64);
}
// This lane's rank in a ballot: the set lanes below it.
__device__ __forceinline__ uint32_t wave_rank(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The length the header at o claims: its ITEM_ntotal when it is sane
// (crc32c_verify_items' rule, item_desc), else 0.  h: the header as read, when
// 48 bytes of the buffer lie at o (room); the second form looks and reads.
__device__ __forceinline__ uint32_t sane_ntotal(const SpanArgs &a, uint64_t o, const ItemHdr &h, bool room) {
    return item_desc(a, o, h, room).sane ? (uint32_t)h.ntotal(a.cfl) : 0u;
}
__device__ __forceinline__ uint32_t sane_ntotal(const SpanArgs &a, uint64_t o) {
    const bool room = o <= a.base_bytes && a.base_bytes - o >= 48;
    ItemHdr h{0u, 0u, 0u, 0u};
    if (room) h = parse_hdr(a.base + o);
    return sane_ntotal(a, o, h, room);
}

// *p0 += the workgroup's sum of a (and p0[1] += that of b): one atomic per
// word and workgroup.  (Same-address atomics serialise in L2, about 8 ns each:
// one per tile with a candidate made a whole-buffer scan of 300 pages 117 ms.)
// Every thread of the block calls it.
__device__ __forceinline__ void block_add64(unsigned long long *p0, uint64_t a, uint64_t b, uint32_t lane) {
    __shared__ unsigned long long sh[2];
    if (threadIdx.x == 0) sh[0] = sh[1] = 0;
    __syncthreads();
    a = wave_sum64(a);
    b = wave_sum64(b);
    if (lane == 0 && (a | b)) {
        atomicAdd(&sh[0], (unsigned long long)a);
        atomicAdd(&sh[1], (unsigned long long)b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sh[0]) atomicAdd(p0, sh[0]);
        if (sh[1]) atomicAdd(p0 + 1, sh[1]);
    }
}

// One piece's tiles in a regions kernel (k_salvage_regions, and
// k_recover_regions of k_recover.h): the kernel finds each round's ranges, one
// per lane, by its own rule; what becomes of them is the same.  w: the piece,
// ending at pe; first: prefix[w] (EMIT); j: the lane.
template <bool EMIT>
struct TileRun {
    const SalvageArgs &s;
    SalvageTile *tiles;
    uint64_t cap, w, pe, first;
    uint32_t j;
    uint64_t scanned = 0;        // this lane's eligible offsets
    uint32_t run = 0, mine = 0;  // tiles written so far (wave-uniform) / counted by this lane
    uint32_t nreg = 0;           // ranges so far (wave-uniform)

    // the tiles of one round's ranges (r, nt tiles, per lane): every range in turn, its tiles by all lanes
    __device__ __forceinline__ void put(const mcrc::SalvageRange &r, uint32_t nt) {
        const uint32_t inc = wave_incl_scan(nt, j);
        unsigned long long m = __ballot(nt != 0);
        while (m) {
            const int src = __ffsll(m) - 1;
            m &= m - 1;
            const uint64_t lo = shfl64(r.lo, src), hi = shfl64(r.hi, src);
            const uint32_t n_r = __shfl(nt, src, 64), at = run + __shfl(inc - nt, src, 64);
            for (uint32_t k = j; k < n_r; k += 64) {
                const mcrc::SalvageRange t = mcrc::salvage_tile(lo, hi, s.ba, k);
                const uint64_t idx = first + at + k;
                if (idx < cap) tiles[idx] = SalvageTile{t.lo, t.hi, pe};
            }
        }
        run += __shfl(inc, 63, 64);
    }
    // EMIT, and the count pass kept all of the piece's ranges: its tiles are cut from those
    __device__ __forceinline__ bool from_kept() {
        if (!EMIT || s.nregs[w] > kSvSlots) return false;
        mcrc::SalvageRange r{0, 0};
        if (j < s.nregs[w]) r = {s.slots[(w * kSvSlots + j) * 2], s.slots[(w * kSvSlots + j) * 2 + 1]};
        put(r, (uint32_t)mcrc::salvage_ntiles(r.lo, r.hi, s.ba));
        return true;
    }
    // one round: this lane's range r (in: it has one).  EMIT: its tiles are
    // written; else counted, and the piece's first kSvSlots ranges kept for the emit pass
    __device__ __forceinline__ void round(mcrc::SalvageRange r, bool in) {
        if (!in) r.hi = r.lo;
        const uint32_t nt = (uint32_t)mcrc::salvage_ntiles(r.lo, r.hi, s.ba);
        if (EMIT) {
            put(r, nt);
            return;
        }
        scanned += r.hi - r.lo;
        mine += nt;
        const unsigned long long hm = __ballot(nt != 0);
        const uint32_t at = nreg + wave_rank(hm);
        if (nt != 0 && at < kSvSlots) {
            s.slots[(w * kSvSlots + at) * 2] = r.lo;
            s.slots[(w * kSvSlots + at) * 2 + 1] = r.hi;
        }
        nreg += (uint32_t)__popcll(hm);
    }
    // behind the piece's last round (the count pass): nregs[w], cnt[w], the lane's share of the scanned
    __device__ __forceinline__ void done(uint32_t *cnt, uint64_t &all_scanned) {
        if (EMIT) return;
        if (j == 0) s.nregs[w] = nreg;
        wave_sum(mine);
        if (j == 0) cnt[w] = mine;
        all_scanned += scanned;
    }
};

// Regions.  One wave per piece [ps, pe).  The piece's list entries are found by
// two binary searches; "entry" 0 of the piece is its head, the bytes in front
// of its first image, and lane j of a round takes entry v: its covered end e
// (the image's end when it covers, else its start), the running maximum of
// the ends up to it (an inclusive scan: a list need not partition the piece,
// and an image that covers may reach past its successors), and the gap from
// there to the next entry, or to the piece's end behind the last one.  The
// gap's eligible offsets (salvage_cut) are cut into tiles (salvage_tile).
//   EMIT false: cnt[w] = the piece's tiles, ctr[kSvScanned] += its eligible offsets;
//     the piece's first kSvSlots ranges are kept (a clean piece has one, its
//     zero tail; a damaged one a few);
//   EMIT true:  the tiles are written from index prefix[w] on, in ascending
//     order: cut from the kept ranges, or for a piece of more ranges than
//     those by going through its entries again (the second pass over a clean
//     page's lists re-read every image's header line: a third of the call).
// a: base, base_bytes, region (= wbuf), cfl.
template <bool EMIT>
__global__ __launch_bounds__(64 * kWalkWaves) void k_salvage_regions(SpanArgs a, SalvageArgs s, uint32_t *cnt,
                                                                     const uint32_t *prefix, SalvageTile *tiles,
                                                                     uint64_t cap) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    if (s.ctr[kSvBad]) return;  // (every thread alike)
    const uint32_t j = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t all_scanned = 0;  // this lane's share of the eligible offsets of the wave's pieces
    for (uint64_t w = (uint64_t)blockIdx.x * kWalkWaves + wave; w < s.nw; w += (uint64_t)gridDim.x * kWalkWaves) {
        const uint64_t ps = w * a.region, pe = mcrc::salvage_piece_end(w, a.region, a.base_bytes);
        TileRun<EMIT> tr{s, tiles, cap, w, pe, EMIT ? prefix[w] : 0, j};
        if (tr.from_kept()) continue;  // (no header is read again)
        uint64_t carry = ps;  // the covered bytes end here (wave-uniform)
        const uint64_t i0 = s.nwalked ? sv_lower_bound(s.walked, s.nwalked, ps) : 0;
        const uint64_t i1 = s.nwalked ? sv_lower_bound(s.walked, s.nwalked, pe) : 0;
        const uint64_t nv = i1 - i0 + 1;  // the head and the entries
        for (uint64_t v0 = 0; v0 < nv; v0 += 64) {
            const uint64_t v = v0 + j;
            const bool in = v < nv;
            uint64_t e = ps, nxt = pe;
            if (in) {
                if (v) {
                    const uint64_t i = i0 + v - 1, o = s.walked[i];
                    e = o;
                    if (s.walked_ok[i]) e = o + sane_ntotal(a, o);
                }
                if (i0 + v < i1) nxt = s.walked[i0 + v];
            }
            uint64_t pm = e;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t t = (uint64_t)__shfl_up((unsigned long long)pm, d, 64);
                if (j >= d && t > pm) pm = t;
            }
            if (carry > pm) pm = carry;
            carry = shfl64(pm, 63);
            tr.round(mcrc::salvage_cut(pm, nxt, ps, pe), in);
        }
        tr.done(cnt, all_scanned);
    }
    if constexpr (!EMIT) block_add64(s.ctr + kSvScanned, all_scanned, 0ull, j);
}

// The header fields of the offset J bytes into a 32-byte window d[0..8) that
// starts 32 bytes behind the offset's piece: nbytes at window bytes J..J+3,
// it_flags at J+6..J+7, nkey at J+9, funnelled out with v_alignbyte_b32 as
// parse_hdr does (no 64-bit shift: k_common.h).
template <int J>
__device__ __forceinline__ mcrc::SalvageHdr sv_fields(const uint32_t (&d)[8]) {
    constexpr int f = J + 6, k = J + 9;
    return {__builtin_amdgcn_alignbyte(d[J / 4 + 1], d[J / 4], J & 3),
            __builtin_amdgcn_alignbyte(d[f / 4 + 1], d[f / 4], f & 3) & 0xffffu,
            __builtin_amdgcn_alignbyte(d[k / 4 + 1], d[k / 4], k & 3) & 0xffu};
}

// The cheap test in front of sv_test: can the offset J bytes into the window
// be sane at all?  50 + nbytes <= room = lim - J, on nbytes alone.  It may pass
// an offset that is not sane (and passes every one where lim - J - 50 wraps,
// in a piece's last 50 bytes); it never stops one that is: sv_test decides.
template <int J>
__device__ __forceinline__ uint32_t sv_pre(const uint32_t (&d)[8], uint32_t lim) {
    const uint32_t nbytes = __builtin_amdgcn_alignbyte(d[J / 4 + 1], d[J / 4], J & 3);
    return nbytes <= lim - (50u + J) ? 1u << J : 0u;
}

// One lane's piece: the 16 offsets P .. P + 15 (from base; P may lie in front
// of it), of which [jlo, jhi) are eligible.  Returns the mask of candidates;
// nts[J] = candidate J's ITEM_ntotal.
struct SvLane {
    uint32_t mask;
    uint64_t work;
};
template <int J, bool NT>
__device__ __forceinline__ void sv_test(const uint32_t (&d)[8], gbyte *gb, int64_t P, int jlo, int jhi, uint64_t pe,
                                        uint32_t cfl, SvLane &out, uint32_t (&nts)[NT ? 16 : 1]) {
    if (J < jlo || J >= jhi) return;
    const mcrc::SalvageHdr h = sv_fields<J>(d);
    const uint64_t o = (uint64_t)(P + J);
    const uint32_t nt = mcrc::salvage_span(h, cfl, pe - o);
    // only a sane header's last two bytes are fetched: they lie inside its piece
    if (nt && mcrc::salvage_has_crlf(h.nbytes) && mcrc::salvage_crlf(gb[o + nt - 2], gb[o + nt - 1])) {
        out.mask |= 1u << J;
        out.work += nt - 32u;
        if constexpr (NT) nts[J] = nt;
    }
}

// The scan.  A wave per tile, many tiles per wave; a tile's aligned 4 KiB
// block is 4 rounds of 64 pieces.  Lane j of a round owns the piece at P: the
// fields of its 16 offsets lie in the two pieces at P + 32 and P + 48, loaded
// as they lie (each holds a header byte of an eligible offset of this lane, so
// neither leaves the bytes the walk's own header reads touch; the second is
// needed, and read, only when an offset from P + 7 on is eligible).  The
// pieces of neighbouring lanes overlap: every byte comes from HBM once and from
// the cache a second time.  (One round's loads at a time: with all four
// rounds' loads issued ahead, 119 VGPRs, a whole-buffer scan was no faster --
// 12.9 against 12.7 ms per 300 pages; the per-offset tests and the dependent
// two-byte fetch of each survivor bound it, not the loads.)
//   EMIT false: tcnt[t] = the tile's candidates; ctr[kSvCand], ctr[kSvWork] += its totals;
//   EMIT true:  tiles with candidates (tpre[t + 1] != tpre[t]) are read again and
//               candidate tpre[t] + r's offset and ntotal written, ascending.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_salvage_scan(SpanArgs a, SalvageArgs s, const SalvageTile *tiles,
                                                      uint32_t ntiles, uint32_t *tcnt, const uint32_t *tpre,
                                                      uint64_t *cand, uint32_t *cand_nt, uint64_t ncap) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t j = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    gbyte *gb = (gbyte *)a.base;
    uint64_t all_cand = 0, all_work = 0;  // this lane's share of the wave's tiles
    for (uint32_t t = blockIdx.x * 4u + wave; t < ntiles; t += gridDim.x * 4u) {
        uint32_t at = 0;
        if (EMIT) {
            at = tpre[t];
            if (tpre[t + 1] == at) continue;
        }
        const SalvageTile T = tiles[t];
        // the block's first byte, from base (negative in the buffer's first block when ba != 0)
        const int64_t blk = (int64_t)((s.ba + T.lo) & ~(uint64_t)(mcrc::kSalvageTile - 1)) - (int64_t)s.ba;
        uint32_t ncand = 0;
        uint64_t work = 0;
#pragma unroll 1
        for (uint32_t it = 0; it < mcrc::kSalvageTile / 1024; ++it) {
            const int64_t P = blk + 16 * (int64_t)(64 * it + j);
            const int64_t dlo = (int64_t)T.lo - P, dhi = (int64_t)T.hi - P;
            const int jlo = dlo > 0 ? (dlo < 16 ? (int)dlo : 16) : 0, jhi = dhi < 16 ? (dhi > 0 ? (int)dhi : 0) : 16;
            SvLane ln{0u, 0ull};
            uint32_t nts[EMIT ? 16 : 1];
            if (jlo < jhi) {
                const uint4 q0 = ld16(gb + (P + 32));
                const uint4 q1 = jhi >= 8 ? ld16(gb + (P + 48)) : make_uint4(0u, 0u, 0u, 0u);
                const uint32_t d[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                // nbytes alone first: a sane image has 50 + nbytes <= room, which one offset
                // in 2^10 of random bytes passes in a 4 MiB wbuf; only those take the full test
                const uint64_t room0 = T.pe - (uint64_t)(P + jlo) + (uint64_t)jlo;  // pe - P
                const uint32_t lim = room0 > 0x80000100ull ? 0x80000100u : (uint32_t)room0;
                uint32_t pre = 0;
#define MCRC_SV_PRE(J) pre |= sv_pre<J>(d, lim)
                MCRC_SV_PRE(0); MCRC_SV_PRE(1); MCRC_SV_PRE(2); MCRC_SV_PRE(3);
                MCRC_SV_PRE(4); MCRC_SV_PRE(5); MCRC_SV_PRE(6); MCRC_SV_PRE(7);
                MCRC_SV_PRE(8); MCRC_SV_PRE(9); MCRC_SV_PRE(10); MCRC_SV_PRE(11);
                MCRC_SV_PRE(12); MCRC_SV_PRE(13); MCRC_SV_PRE(14); MCRC_SV_PRE(15);
#undef MCRC_SV_PRE
#define MCRC_SV_TEST(J) \
    if (pre & (1u << J)) sv_test<J, EMIT>(d, gb, P, jlo, jhi, T.pe, a.cfl, ln, nts)
                if (pre) {
                    MCRC_SV_TEST(0); MCRC_SV_TEST(1); MCRC_SV_TEST(2); MCRC_SV_TEST(3);
                    MCRC_SV_TEST(4); MCRC_SV_TEST(5); MCRC_SV_TEST(6); MCRC_SV_TEST(7);
                    MCRC_SV_TEST(8); MCRC_SV_TEST(9); MCRC_SV_TEST(10); MCRC_SV_TEST(11);
                    MCRC_SV_TEST(12); MCRC_SV_TEST(13); MCRC_SV_TEST(14); MCRC_SV_TEST(15);
                }
#undef MCRC_SV_TEST
            }
            const uint32_t c = __popc(ln.mask);
            if (!EMIT) {
                ncand += c;
                work += ln.work;
                continue;
            }
            const uint32_t inc = wave_incl_scan(c, j);
            uint32_t idx = at + inc - c;
#pragma unroll
            for (int J = 0; J < 16; ++J)
                if (ln.mask & (1u << J)) {
                    if (idx < ncap) {
                        cand[idx] = (uint64_t)(P + J);
                        cand_nt[idx] = nts[J];
                    }
                    ++idx;
                }
            at += __shfl(inc, 63, 64);
        }
        if (!EMIT) {
            all_cand += ncand;
            all_work += work;
            wave_sum(ncand);
            if (j == 0) tcnt[t] = ncand;
        }
    }
    if constexpr (!EMIT) block_add64(s.ctr + kSvCand, all_cand, all_work, j);  // (kSvWork = kSvCand + 1)
}

// What the pick needs to keep suspects (crc32c_triage_pages): the walk's list
// and the scan of its per-piece counts (piece w's entries are [wpre[w],
// wpre[w + 1])), the per-piece counts of the found, and the kind bytes.  The
// salvage's and the recover call's launches pass it empty.
struct PickSuspects {
    const uint64_t *walked;
    const uint32_t *wpre;
    uint32_t *fcnt;
    uint8_t *okind;
};

// The pick.  One wave per piece over its candidates (two binary searches), 64
// a round; the verified ones are gone through in order by the whole wave (the
// state, the end of the last image kept, is wave-uniform), and a candidate is
// kept (found) when it starts at or after that end.
// SUSPECTS: a failing candidate is picked too, as a suspect, when
//   it starts at or after the end that the verified candidates below it have
//     produced (each lane keeps the end as of the lanes before it: `mine`; a
//     suspect never moves the end, its length is not proven);
//   it is no entry of the walk's list (a walked entry with verdict 0 that is
//     itself a failing candidate is in the list already, as kind 0): a search
//     in the piece's own entries.
// (Outside the covered set it is by being a candidate: the scan looks at
// eligible offsets only.)  Without SUSPECTS none of that is compiled in.
//   EMIT false: cnt[w] = the piece's picked candidates (SUSPECTS: and
//               t.fcnt[w] = the found among them);
//   EMIT true:  picked candidate prefix[w] + r is written to out, when below
//               cap (SUSPECTS: and its kind, kKindSalvaged or kKindSuspect, to t.okind).
template <bool EMIT, bool SUSPECTS>
__global__ __launch_bounds__(64 * kWalkWaves) void k_salvage_pick(const uint64_t *cand, const uint32_t *cand_nt,
                                                                  const uint8_t *ok, uint64_t ncand, uint64_t wbuf,
                                                                  uint64_t base_bytes, uint64_t nw, uint32_t *cnt,
                                                                  const uint32_t *prefix, uint64_t *out, uint64_t cap,
                                                                  PickSuspects t) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t j = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t w = (uint64_t)blockIdx.x * kWalkWaves + wave; w < nw; w += (uint64_t)gridDim.x * kWalkWaves) {
        const uint64_t ps = w * wbuf, pe = mcrc::salvage_piece_end(w, wbuf, base_bytes);
        const uint64_t c0 = sv_lower_bound(cand, ncand, ps), c1 = sv_lower_bound(cand, ncand, pe);
        const uint64_t first = EMIT ? prefix[w] : 0;
        uint64_t i0 = 0, nwk = 0;  // the piece's walked entries
        if constexpr (SUSPECTS) {
            i0 = t.wpre[w];
            nwk = t.wpre[w + 1] - i0;
        }
        uint64_t end = 0;
        uint32_t picked = 0, kept = 0;
        for (uint64_t cc = c0; cc < c1; cc += 64) {
            const uint64_t i = cc + j;
            const bool in = i < c1;
            const uint64_t o = in ? cand[i] : 0;
            const uint32_t nt = in ? cand_nt[i] : 0u;
            const bool good = in && ok[in ? i : c0] != 0;
            uint64_t mine = end;  // the end as of the lanes before this one
            bool keep = false, suspect = false;
            unsigned long long m = __ballot(good);
            while (m) {
                const int src = __ffsll(m) - 1;
                m &= m - 1;
                const uint64_t so = shfl64(o, src);
                if (so >= end) {
                    end = so + __shfl(nt, src, 64);
                    keep |= (int)j == src;
                    if (SUSPECTS && (int)j > src) mine = end;
                }
            }
            unsigned long long pm = __ballot(keep);  // the picked: the kept ...
            if constexpr (SUSPECTS) {  // ... and the suspects
                suspect = in && !good && o >= mine;
                if (suspect && nwk) {
                    const uint64_t k = sv_lower_bound(t.walked + i0, nwk, o);
                    suspect = !(k < nwk && t.walked[i0 + k] == o);
                }
                kept += (uint32_t)__popcll(pm);
                pm |= __ballot(suspect);
            }
            if (EMIT && (keep || suspect)) {
                const uint64_t idx = first + picked + wave_rank(pm);
                if (idx < cap) {
                    out[idx] = o;
                    if constexpr (SUSPECTS) t.okind[idx] = keep ? kKindSalvaged : kKindSuspect;
                }
            }
            picked += (uint32_t)__popcll(pm);
        }
        if (!EMIT && j == 0) {
            cnt[w] = picked;
            if constexpr (SUSPECTS) t.fcnt[w] = kept;
        }
    }
}

}  // namespace mcrc_dev
