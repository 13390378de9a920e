// k_triage.h -- crc32c_triage_pages: crc32c_recover_pages with the candidates
// whose stored CRC does not match listed too (kind 6, CRC32C_ITEM_SUSPECT), so
// that a data-damaged image behind a header that ended its wbuf's walk can be
// handed to crc32c_repair_items.
//
// The walk, the regions, the scan and the candidates' CRCs are the recover
// call's own kernels (k_recover.h, k_salvage.h); two things differ:
//   k_triage_pick   k_salvage_pick that also keeps the failing candidates the
//                   cursor of the rule reaches, with a kind byte beside each
//                   offset picked;
//   k_triage_merge  k_recover_merge over the walk's list and the picked list,
//                   a picked entry's kind taken from that byte.
// (Their own kernels: k_salvage_pick's and k_recover_merge's instruction
// streams are kept as they are, as for k_recover_regions.)
#pragma once

#include "k_recover.h"

namespace mcrc_dev {

constexpr uint8_t kKindSuspect = 6;  // CRC32C_ITEM_SUSPECT

// The pick.  One wave per piece over its candidates, 64 a round, as in
// k_salvage_pick: the verified ones are gone through in order by the whole
// wave, and one is kept (found) when it starts at or after `end`, the end of
// the last one kept.  A failing candidate is picked as a suspect when
//   it starts at or after the end that the verified candidates below it have
//     produced (each lane keeps the end as of the lanes before it: `mine`; a
//     suspect never moves the end, its length is not proven);
//   it is no entry of the walk's list (a walked entry with verdict 0 that is
//     itself a failing candidate is in the list already, as kind 0): a search
//     in the piece's own entries [wpre[w], wpre[w + 1]).
// (Outside the covered set it is by being a candidate: the scan looks at
// eligible offsets only.)
//   EMIT false: cnt[w] = the piece's picked candidates, fcnt[w] = the found among them;
//   EMIT true:  picked candidate prefix[w] + r is written to out and its kind
//               (kKindSalvaged or kKindSuspect) to okind, when below cap.
template <bool EMIT>
__global__ __launch_bounds__(64 * kWalkWaves) void k_triage_pick(const uint64_t *cand, const uint32_t *cand_nt,
                                                                 const uint8_t *ok, uint64_t ncand, uint64_t wbuf,
                                                                 uint64_t base_bytes, uint64_t nw,
                                                                 const uint64_t *walked, const uint32_t *wpre,
                                                                 uint32_t *cnt, uint32_t *fcnt, const uint32_t *prefix,
                                                                 uint64_t *out, uint8_t *okind, uint64_t cap) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint32_t j = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t w = (uint64_t)blockIdx.x * kWalkWaves + wave; w < nw; w += (uint64_t)gridDim.x * kWalkWaves) {
        const uint64_t ps = w * wbuf, pe = mcrc::salvage_piece_end(w, wbuf, base_bytes);
        const uint64_t c0 = sv_lower_bound(cand, ncand, ps), c1 = sv_lower_bound(cand, ncand, pe);
        const uint64_t first = EMIT ? prefix[w] : 0;
        const uint64_t i0 = wpre[w], nwk = wpre[w + 1] - i0;  // the piece's walked entries
        uint64_t end = 0;
        uint32_t picked = 0, kept = 0;
        for (uint64_t cc = c0; cc < c1; cc += 64) {
            const uint64_t i = cc + j;
            const bool in = i < c1;
            const uint64_t o = in ? cand[i] : 0;
            const uint32_t nt = in ? cand_nt[i] : 0u;
            const bool good = in && ok[in ? i : c0] != 0;
            uint64_t mine = end;  // the end as of the lanes before this one
            bool keep = false;
            unsigned long long m = __ballot(good);
            while (m) {
                const int src = __ffsll(m) - 1;
                m &= m - 1;
                const uint64_t so = shfl64(o, src);
                if (so >= end) {
                    end = so + __shfl(nt, src, 64);
                    keep |= (int)j == src;
                    if ((int)j > src) mine = end;
                }
            }
            bool suspect = in && !good && o >= mine;
            if (suspect && nwk) {
                const uint64_t k = sv_lower_bound(walked + i0, nwk, o);
                suspect = !(k < nwk && walked[i0 + k] == o);
            }
            const unsigned long long km = __ballot(keep), pm = km | __ballot(suspect);
            if (EMIT && (keep || suspect)) {
                const uint64_t idx = first + picked +
                                     __builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0u));
                if (idx < cap) {
                    out[idx] = o;
                    okind[idx] = keep ? kKindSalvaged : kKindSuspect;
                }
            }
            picked += (uint32_t)__popcll(pm);
            kept += (uint32_t)__popcll(km);
        }
        if (!EMIT && j == 0) {
            cnt[w] = picked;
            fcnt[w] = kept;
        }
    }
}

// The merge: k_recover_merge with the picked list (found images and suspects
// together, ascending per piece and over the buffer, no offset of it in the
// walk's list) in the place of the images found.  ppre: the scan of the
// pick's per-piece counts, nullptr when nothing was picked; pkind: the kind
// byte of each picked entry.  A picked entry's length is the ITEM_ntotal the
// scan kept beside its candidate (never 0: a candidate is sane).
__global__ __launch_bounds__(256) void k_triage_merge(SpanArgs a, const uint64_t *walked, const uint8_t *wok,
                                                      const uint32_t *wpre, uint64_t nw, const uint64_t *picked,
                                                      const uint8_t *pkind, const uint32_t *ppre,
                                                      const uint64_t *cand, const uint32_t *cand_nt, uint64_t ncand,
                                                      uint64_t per, RecoverOut out) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint64_t nwalked = wpre[nw], np = ppre ? ppre[nw] : 0, n = nwalked + np;
    const uint64_t t1 = (blockIdx.x + 1ull) * per < n ? (blockIdx.x + 1ull) * per : n;
    uint64_t k = 0;  // the piece of this thread's last walked entry is k - 1 (0: none yet)
    for (uint64_t t = blockIdx.x * per + threadIdx.x; t < t1; t += blockDim.x) {
        const bool w = t < nwalked;
        const uint64_t i = w ? t : t - nwalked;
        const uint64_t o = w ? walked[i] : picked[i];
        uint64_t at = i;
        if (w) {
            if (k == 0) k = rc_piece_end(wpre, nw, i);
            while (wpre[k] <= i) ++k;  // (wpre[nw] = nwalked > i: k stays <= nw)
            if (ppre) at += ppre[k - 1] + sv_lower_bound(picked + ppre[k - 1], ppre[k] - ppre[k - 1], o);
        } else {
            at += sv_lower_bound(walked, nwalked, o);
        }
        if (at >= out.cap) continue;
        uint8_t kind;
        uint32_t len;
        if (!w) {
            kind = pkind[i];
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
