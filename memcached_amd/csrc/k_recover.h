// k_recover.h -- crc32c_recover_pages and crc32c_triage_pages: the page walk,
// its verify and the salvage in one call, the lists passed from stage to stage
// on the device.
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
//   k_recover_merge    the walk's entries and the picked ones, both ascending
//                      and disjoint, merged into one list with kind and lens.
// crc32c_triage_pages is the same call with the candidates whose stored CRC
// does not match listed too (kind 6, CRC32C_ITEM_SUSPECT), so that a
// data-damaged image behind a header that ended its wbuf's walk can be handed
// to crc32c_repair_items: its pick keeps the suspects (k_salvage_pick's
// SUSPECTS, k_salvage.h) and writes a kind byte beside each offset picked,
// which the merge takes in the place of the constant kind 4.
#pragma once

#include "k_salvage.h"

namespace mcrc_dev {

// Regions from the walk.  One wave per piece, lane j of a round an entry, as
// in k_salvage_regions, with the same outputs (TileRun: cnt, ctr[kSvScanned],
// the kept ranges / the tiles from prefix[w] on).  Piece w's entries are
// [wpre[w], wpre[w + 1]); the walk starts at the piece's first byte and each
// entry starts where its predecessor's ITEM_ntotal ends, so the covered ends
// ascend by themselves (no running maximum) and the uncovered gaps are
//   a piece without entries: all of it;
//   behind an entry with verdict 0: from its start to the next entry, or to
//     the piece's end behind the last one;
//   behind the last entry when its verdict is not 0: from its image's end (the
//     one header read of the piece) to the piece's end.
// (Two kernels, not one: the salvage's takes a running maximum over a list
// that need not partition the piece and reads a header per image.)
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
        TileRun<EMIT> tr{s, tiles, cap, w, pe, EMIT ? prefix[w] : 0, j};
        if (tr.from_kept()) continue;
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
                    if (s.walked_ok[i]) e = i + 1 == i1 ? o + sane_ntotal(a, o) : nxt;
                }
            }
            tr.round(mcrc::salvage_cut(e, nxt, ps, pe), in);
        }
        tr.done(cnt, all_scanned);
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

// The merge.  One thread per entry of either list, the walk's and the picked
// (the images found; in a triage the suspects with them: ascending per piece
// and over the buffer, no offset of it in the walk's list); its place in the
// merged list is its own index plus the entries of the other list below it
// (both lists ascend over the whole buffer, and no offset is in both).
// Workgroup b takes the entries [b * per, (b + 1) * per) of the walk's list
// followed by the picked, a thread every 256th of them, so a thread's walked
// entries ascend and it finds its first entry's piece by a search in wpre and
// the later ones' by stepping on from there.  A walked entry's rank among the
// picked is a search among its own piece's (fpre: the scan of the pick's
// per-piece counts; a piece without damage has none); a picked entry is
// searched for in the whole of the walk's list (they are few).
// Only entries that land below out.cap go on to their kind and length:
//   a walked entry: its verdict; with a verdict and a successor in its piece
//     the successor's offset minus its own (no header read), else
//     sane_ntotal of its header;
//   a picked entry: pkind's byte, or with pkind == nullptr (no suspects were
//     asked for) kKindSalvaged; the ITEM_ntotal the scan kept beside its
//     candidate (never 0: a candidate is sane).
// fpre: nullptr when nothing was picked.  a: base, base_bytes, region (= wbuf), cfl.
__global__ __launch_bounds__(256) void k_recover_merge(SpanArgs a, const uint64_t *walked, const uint8_t *wok,
                                                       const uint32_t *wpre, uint64_t nw, const uint64_t *found,
                                                       const uint8_t *pkind, const uint32_t *fpre,
                                                       const uint64_t *cand, const uint32_t *cand_nt, uint64_t ncand,
                                                       uint64_t per, RecoverOut out) {
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
        uint8_t kind;
        uint32_t len;
        if (!w) {
            kind = pkind ? pkind[i] : kKindSalvaged;
            len = cand_nt[sv_lower_bound(cand, ncand, o)];
        } else if ((kind = wok[i]) != 0 && wpre[k] != i + 1) {
            len = (uint32_t)(walked[i + 1] - o);
        } else {
            len = sane_ntotal(a, o);
        }
        out.offsets[at] = o;
        out.lens[at] = len;
        out.kind[at] = kind;
    }
}

}  // namespace mcrc_dev
