// shim_triage.h -- the pick crc32c_triage_pages runs in the place of the
// recover call's: k_salvage_pick with the suspects kept (k_salvage.h).  The
// rest of its body is recover_pages itself (shim_recover.h), which calls this
// when it is asked for the suspects and hands the merge the kind bytes.
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
    r.launch_pick<true>(p->picked, r.nc, mcrc_dev::PickSuspects{walked, r.wpre, fcnt, p->kind});
    scan32(r.st, fcnt, nw, p->fpre);
    HIP_OK(hipGetLastError());
    // the two totals: picked, found
    HIP_OK(hipMemcpyAsync(r.h32, r.ppre + nw, 4, hipMemcpyDeviceToHost, r.st));
    HIP_OK(hipMemcpyAsync(r.h32 + 1, p->fpre + nw, 4, hipMemcpyDeviceToHost, r.st));
    return CRC32C_OK;
}

}  // namespace
