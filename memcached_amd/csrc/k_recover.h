// k_recover.h -- crc32c_recover_pages: the page walk, its verify and the
// salvage in one call, the lists passed from stage to stage on the device.
//
// The walk (k_walk.h) leaves its offsets, verdicts and the scan of its
// per-piece counts (wpre: piece w's entries are [wpre[w], wpre[w + 1])) in
// scratch.  Two things follow from the list being the library's own walk of
// the same bytes, and the kernels here rely on both (tests/test_recover_model.py
// pins them on the CPU): a verdict that is not 0 means a sane header, and inside
// a piece an entry's image ends where the next entry starts.
//   k_recover_regions  k_salvage_regions' work with the covered set taken from
//                      the walk: no order check, no search, one header read
//                      per piece instead of one per image;
//   (scan, candidates and pick: the salvage's own kernels)
//   k_recover_merge    the walk's entries and the images found, both ascending
//                      and disjoint, merged into one list with kind and lens.
#pragma once

#include "k_salvage.h"

namespace mcrc_dev {

constexpr uint8_t kKindSalvaged = 4;  // CRC32C_ITEM_SALVAGED

// Regions from the walk.  One wave per piece, lane j of a round an entry, as
// in k_salvage_regions, with the same outputs (cnt, ctr[kSvScanned], the kept
// ranges / the tiles from prefix[w] on).  Piece w's entries are [wpre[w],
// wpre[w + 1]); the walk starts at the piece's first byte and each entry
// starts where its predecessor's ITEM_ntotal ends, so the covered ends ascend
// by themselves (no running maximum) and the uncovered gaps are
//   a piece without entries: all of it;
//   behind an entry with verdict 0: from its start to the next entry, or to
//     the piece's end behind the last one;
//   behind the last entry when its verdict is not 0: from its image's end (the
//     one header read of the piece) to the piece's end.
// (Its own kernel: k_salvage_regions' instruction stream is kept as it is, and
// calling one inlined body from both changed that kernel's schedule.)
// a: base, base_bytes, region (= wbuf), cfl.  s: walked, walked_ok, nw, ba, ctr, slots, nregs.
template <bool EMIT>
__global__ __launch_bounds__(64 * kWalkWaves) void k_recover_regions(SpanArgs a, SalvageArgs s, const uint32_t *wpre,
                                                                     uint32_t *cnt, const uint32_t *prefix,
                                                                     SalvageTile *tiles, uint64_t cap) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t j = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t all_scanned = 0;  // this lane's share of the eligible offsets of the wave's pieces
    for (uint64_t w = (uint64_t)blockIdx.x * kWalkWaves + wave; w < s.nw; w += (uint64_t)gridDim.x * kWalkWaves) {
        const uint64_t ps = w * a.region, pe = mcrc::salvage_piece_end(w, a.region, a.base_bytes);
        const uint64_t first = EMIT ? prefix[w] : 0;
        uint64_t scanned = 0;
        uint32_t run = 0, mine = 0;  // tiles written so far (wave-uniform) / counted by this lane
        uint32_t nreg = 0;           // ranges so far (wave-uniform)
        // the tiles of one round's ranges (r, nt tiles, per lane): every range in turn, its tiles by all lanes
        auto put = [&](const mcrc::SalvageRange &r, uint32_t nt) {
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
        };
        if (EMIT && s.nregs[w] <= kSvSlots) {  // the count pass kept them all
            mcrc::SalvageRange r{0, 0};
            if (j < s.nregs[w]) r = {s.slots[(w * kSvSlots + j) * 2], s.slots[(w * kSvSlots + j) * 2 + 1]};
            put(r, (uint32_t)mcrc::salvage_ntiles(r.lo, r.hi, s.ba));
            continue;
        }
        const uint64_t i0 = wpre[w], i1 = wpre[w + 1];
        // the head (the bytes in front of the first entry: none, unless the piece has no entry) and the entries
        const uint64_t nv = i1 - i0 + 1;
        for (uint64_t v0 = 0; v0 < nv; v0 += 64) {
            const uint64_t v = v0 + j;
            const bool in = v < nv;
            uint64_t e = ps, nxt = pe;
            if (in) {
                if (i0 + v < i1) nxt = s.walked[i0 + v];
                if (v) {
                    const uint64_t i = i0 + v - 1, o = s.walked[i];
                    e = o;
                    if (s.walked_ok[i]) {
                        e = nxt;
                        if (i + 1 == i1) {
                            const bool hdr_ok = o <= a.base_bytes && a.base_bytes - o >= 48;
                            ItemHdr h{0u, 0u, 0u, 0u};
                            if (hdr_ok) h = parse_hdr(a.base + o);
                            e = item_desc(a, o, h, hdr_ok).sane ? o + h.ntotal(a.cfl) : o;
                        }
                    }
                }
            }
            mcrc::SalvageRange r = mcrc::salvage_cut(e, nxt, ps, pe);
            if (!in) r.hi = r.lo;
            const uint32_t nt = (uint32_t)mcrc::salvage_ntiles(r.lo, r.hi, s.ba);
            if (EMIT) {
                put(r, nt);
                continue;
            }
            scanned += r.hi - r.lo;
            mine += nt;
            // the piece's first kSvSlots ranges are kept for the emit pass
            const unsigned long long hm = __ballot(nt != 0);
            const uint32_t at = nreg + __builtin_amdgcn_mbcnt_hi((uint32_t)(hm >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo((uint32_t)hm, 0u));
            if (nt != 0 && at < kSvSlots) {
                s.slots[(w * kSvSlots + at) * 2] = r.lo;
                s.slots[(w * kSvSlots + at) * 2 + 1] = r.hi;
            }
            nreg += (uint32_t)__popcll(hm);
        }
        if (!EMIT && j == 0) s.nregs[w] = nreg;
        if (!EMIT) {
            wave_sum(mine);
            if (j == 0) cnt[w] = mine;
            all_scanned += scanned;
        }
    }
    if constexpr (!EMIT) block_add64(s.ctr + kSvScanned, all_scanned, 0ull, j);
}

struct RecoverOut {
    uint64_t *offsets;
    uint32_t *lens;
    uint8_t *kind;
    uint64_t cap;  // entries written: the merged list's first cap
};

// The first k of [1, n] with pre[k] > i (pre ascending, pre[n] > i).
__device__ __forceinline__ uint64_t rc_piece_end(const uint32_t *pre, uint64_t n, uint64_t i) {
    uint64_t lo = 1, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (pre[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The merge.  One thread per entry of either list; its place in the merged
// list is its own index plus the entries of the other list below it (both
// lists ascend over the whole buffer, and no offset is in both).  Workgroup b
// takes the entries [b * per, (b + 1) * per) of the walk's list followed by
// the images found, a thread every 256th of them, so a thread's walked
// entries ascend and it finds its first entry's piece by a search in wpre and
// the later ones' by stepping on from there.  A walked entry's rank among the
// images found is a search among its own piece's (fpre: the scan of the
// pick's per-piece counts; a piece without damage has none); an image found
// is searched for in the whole of the walk's list (they are few).
// Only entries that land below out.cap go on to their length:
//   a walked entry with a verdict and a successor in its piece: the successor's
//     offset minus its own (no header read);
//   any other walked entry: ITEM_ntotal from its header when that is sane
//     (crc32c_verify_items' rule, item_desc), else 0;
//   an image found: the ITEM_ntotal the scan kept beside its candidate.
// fpre: nullptr when nothing was found.  a: base, base_bytes, region (= wbuf), cfl.
__global__ __launch_bounds__(256) void k_recover_merge(SpanArgs a, const uint64_t *walked, const uint8_t *wok,
                                                       const uint32_t *wpre, uint64_t nw, const uint64_t *found,
                                                       const uint32_t *fpre, const uint64_t *cand,
                                                       const uint32_t *cand_nt, uint64_t ncand, uint64_t per,
                                                       RecoverOut out) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint64_t nwalked = wpre[nw], nf = fpre ? fpre[nw] : 0, n = nwalked + nf;
    const uint64_t t1 = (blockIdx.x + 1ull) * per < n ? (blockIdx.x + 1ull) * per : n;
    uint64_t k = 0;  // the piece of this thread's last walked entry is k - 1 (0: none yet)
    for (uint64_t t = blockIdx.x * per + threadIdx.x; t < t1; t += blockDim.x) {
        const bool w = t < nwalked;
        const uint64_t i = w ? t : t - nwalked;
        const uint64_t o = w ? walked[i] : found[i];
        uint64_t at = i;
        if (w) {
            if (k == 0) k = rc_piece_end(wpre, nw, i);
            while (wpre[k] <= i) ++k;  // (wpre[nw] = nwalked > i: k stays <= nw)
            if (fpre) at += fpre[k - 1] + sv_lower_bound(found + fpre[k - 1], fpre[k] - fpre[k - 1], o);
        } else {
            at += sv_lower_bound(walked, nwalked, o);
        }
        if (at >= out.cap) continue;
        uint8_t kind = kKindSalvaged;
        uint32_t len;
        if (!w) {
            len = cand_nt[sv_lower_bound(cand, ncand, o)];
        } else if ((kind = wok[i]) != 0 && wpre[k] != i + 1) {
            len = (uint32_t)(walked[i + 1] - o);
        } else {
            const bool hdr_ok = o <= a.base_bytes && a.base_bytes - o >= 48;
            ItemHdr h{0u, 0u, 0u, 0u};
            if (hdr_ok) h = parse_hdr(a.base + o);
            len = item_desc(a, o, h, hdr_ok).sane ? (uint32_t)h.ntotal(a.cfl) : 0u;
        }
        out.offsets[at] = o;
        out.lens[at] = len;
        out.kind[at] = kind;
    }
}

}  // namespace mcrc_dev
