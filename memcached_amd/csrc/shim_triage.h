// shim_triage.h -- the two stages crc32c_triage_pages runs in the place of
// the recover call's pick and merge (k_triage.h): the rest of its body is
// recover_pages itself (shim_recover.h), which calls these when it is asked
// for the suspects.  crc32c_recover_pages launches neither.
#pragma once

namespace {

static_assert(mcrc_dev::kKindSuspect == CRC32C_ITEM_SUSPECT, "the pick writes the header's kind");

// What the pick leaves on the device: the picked list (found images and
// suspects, ascending), a kind byte per entry, and the scans of the per-piece
// counts of the picked (r.ppre) and of the found among them (fpre).
struct TriagePick {
    uint64_t *picked = nullptr;
    uint8_t *kind = nullptr;
    uint32_t *fpre = nullptr;
};

// r.candidates() has run.  The found counts take the words of the regions'
// nregs, free since the scan's tiles were cut.
int triage_pick(SalvageRun &r, const uint64_t *walked, TriagePick *p) {
    Device &d = r.d;
    const uint64_t nw = r.s.nw;
    p->picked = d.sv_out.reserve(r.nc * 8);
    p->kind = d.tr_kind.reserve(r.nc);
    p->fpre = d.tr_fpre.reserve((nw + 2) * 4);
    if (!p->picked || !p->kind || !p->fpre) return CRC32C_ENOMEM;
    uint32_t *fcnt = r.pcnt + nw + 1;
    auto launch = [&](auto kern, uint32_t *cnt, uint32_t *fc, const uint32_t *pre, uint64_t *o, uint8_t *k,
                      uint64_t cap) {
        hipLaunchKernelGGL(kern, r.pgrid, r.pblock, 0, r.st, (const uint64_t *)r.cand, (const uint32_t *)r.cand_nt,
                           (const uint8_t *)r.cok, r.nc, r.a.region, r.a.base_bytes, nw, walked, r.wpre, cnt, fc, pre,
                           o, k, cap);
    };
    launch(mcrc_dev::k_triage_pick<false>, r.pcnt, fcnt, nullptr, nullptr, nullptr, 0);
    hipLaunchKernelGGL(mcrc_dev::k_scan32, dim3(1), dim3(1024), 0, r.st, (const uint32_t *)r.pcnt, nw, r.ppre);
    hipLaunchKernelGGL(mcrc_dev::k_scan32, dim3(1), dim3(1024), 0, r.st, (const uint32_t *)fcnt, nw, p->fpre);
    launch(mcrc_dev::k_triage_pick<true>, nullptr, nullptr, r.ppre, p->picked, p->kind, r.nc);
    HIP_OK(hipGetLastError());
    // the two totals: picked, found
    HIP_OK(hipMemcpyAsync(r.h32, r.ppre + nw, 4, hipMemcpyDeviceToHost, r.st));
    HIP_OK(hipMemcpyAsync(r.h32 + 1, p->fpre + nw, 4, hipMemcpyDeviceToHost, r.st));
    return CRC32C_OK;
}

// p: nullptr when nothing was picked (the walk's entries alone)
int triage_merge(SalvageRun &r, const mcrc_dev::SpanArgs &a, const uint64_t *woffs, const uint8_t *wok,
                 const TriagePick *p, dim3 grid, uint64_t per, const mcrc_dev::RecoverOut &out) {
    hipLaunchKernelGGL(mcrc_dev::k_triage_merge, grid, dim3(256), 0, r.st, a, woffs, wok, r.wpre, r.s.nw,
                       (const uint64_t *)(p ? p->picked : nullptr), (const uint8_t *)(p ? p->kind : nullptr),
                       p ? (const uint32_t *)r.ppre : (const uint32_t *)nullptr, (const uint64_t *)r.cand,
                       (const uint32_t *)r.cand_nt, r.nc, per, out);
    HIP_OK(hipGetLastError());
    return CRC32C_OK;
}

}  // namespace
