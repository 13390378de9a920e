// shim_salvage.h -- the salvage's stages over device-resident inputs
// (SalvageRun: the regions from the walk's lists, the scan of the eligible
// bytes, the candidates' CRCs through the item runners, the pick) and
// salvage_pages, the body of crc32c_salvage_pages, which stages a host call's
// inputs and runs them (k_salvage.h; the contract: include/crc32c_batch.h).
// crc32c_recover_pages runs the same stages behind its own walk (shim_recover.h).
#pragma once

namespace {

static_assert(mcrc::kSalvageWorkMax == CRC32C_SALVAGE_WORK_MAX, "the work bound's factor is the header's");

// One salvage on `st`: the buffer and the lists are device memory.  Each stage
// enqueues its kernels and reads back the one count that sizes the next:
//   regions()     the tiles (what the scan's scratch is sized by; a list that
//                 fails its check ends the call there) and the eligible offsets;
//   scan()        the candidates and their work (none, or past the bound, ends
//                 the call; else they size the verify);
//   candidates()  their offsets and ITEM_ntotals written out, their CRCs checked;
//   pick()        the images found per piece counted and scanned (ppre[nw] is
//                 their number, left on the device) and, with a cap, written.
// wpre (crc32c_recover_pages): the scan of the walk's own per-piece counts; the
// regions then take the covered set from the walk (k_recover_regions).
struct SalvageRun {
    Device &d;
    hipStream_t st;
    mcrc_dev::SpanArgs a;  // base, base_bytes, region (= wbuf), cfl
    mcrc_dev::SalvageArgs s{};
    const uint32_t *wpre = nullptr;
    dim3 pgrid, pblock, sgrid;
    unsigned long long *h = nullptr;  // the counters' pinned twin + a count
    uint32_t *h32 = nullptr, *pcnt = nullptr, *ppre = nullptr;
    mcrc_dev::SalvageTile *tiles = nullptr;
    uint32_t *tcnt = nullptr, *tpre = nullptr, ntiles = 0;
    uint64_t *cand = nullptr;
    uint32_t *cand_nt = nullptr;
    uint8_t *cok = nullptr;
    uint64_t sc = 0, nc = 0, work = 0;  // scanned, candidates, their spans

    // cnt, pre, slots: the per-piece counts, their scan and the ranges the
    // regions' count pass keeps
    int init(const mcrc_dev::SpanArgs &args, const uint64_t *walked, const uint8_t *walked_ok, uint64_t nwalked,
             uint64_t nw, DevBuf<uint32_t> &cnt, DevBuf<uint32_t> &pre, DevBuf<uint64_t> &slots) {
        a = args;
        h = d.sv_host.reserve(8 * sizeof(unsigned long long));
        pcnt = cnt.reserve((2 * nw + 2) * 4);
        ppre = pre.reserve((nw + 2) * 4);
        s.slots = slots.reserve((size_t)nw * mcrc_dev::kSvSlots * 16);
        s.nregs = pcnt ? pcnt + nw + 1 : nullptr;
        s.ctr = d.sv_ctr.reserve(mcrc_dev::kSvWords * sizeof(unsigned long long));
        if (!h || !pcnt || !ppre || !s.ctr || !s.slots) return CRC32C_ENOMEM;
        h32 = (uint32_t *)(h + mcrc_dev::kSvWords);
        s.walked = walked;
        s.walked_ok = walked_ok;
        s.nwalked = nwalked;
        s.nw = nw;
        s.ba = (uint32_t)((uintptr_t)a.base & (mcrc::kSalvageTile - 1));
        pgrid = dim3(mcrc::walk_grid(nw));
        pblock = dim3(64 * mcrc_dev::kWalkWaves);
        return CRC32C_OK;
    }

    template <bool EMIT>
    void launch_regions(uint32_t *cnt, const uint32_t *prefix, mcrc_dev::SalvageTile *out, uint64_t cap) {
        if (wpre)
            hipLaunchKernelGGL(mcrc_dev::k_recover_regions<EMIT>, pgrid, pblock, 0, st, a, s, wpre, cnt, prefix, out,
                               cap);
        else
            hipLaunchKernelGGL(mcrc_dev::k_salvage_regions<EMIT>, pgrid, pblock, 0, st, a, s, cnt, prefix, out, cap);
    }

    // check: a caller's device list is checked first (CRC32C_EINVAL when it fails)
    int regions(bool check) {
        HIP_OK(hipMemsetAsync(s.ctr, 0, mcrc_dev::kSvWords * sizeof(unsigned long long), st));
        if (check)
            hipLaunchKernelGGL(mcrc_dev::k_salvage_check, dim3(mcrc::final_grid(s.nwalked)), dim3(256), 0, st, s,
                               a.base_bytes);
        launch_regions<false>(pcnt, nullptr, nullptr, 0);
        scan32(st, pcnt, s.nw, ppre);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(h, s.ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h32, ppre + s.nw, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (h[mcrc_dev::kSvBad]) return CRC32C_EINVAL;
        sc = h[mcrc_dev::kSvScanned];
        ntiles = *h32;
        g_last_kernel_ms = 0.0f;  // (no scan ran yet: not the time of an earlier call)
        return CRC32C_OK;
    }

    int scan() {
        tiles = d.sv_tiles.reserve((size_t)ntiles * sizeof(mcrc_dev::SalvageTile));
        tcnt = d.sv_tcnt.reserve((size_t)ntiles * 4);
        tpre = d.sv_tpre.reserve(((size_t)ntiles + 1) * 4);
        if (!tiles || !tcnt || !tpre) return CRC32C_ENOMEM;
        launch_regions<true>(nullptr, ppre, tiles, ntiles);
        sgrid = dim3((unsigned)std::min<uint64_t>(((uint64_t)ntiles + 3) / 4, (uint64_t)std::max(d.cus, 1) * 8));
        HIP_OK(hipEventRecord(d.ev0, st));
        hipLaunchKernelGGL(mcrc_dev::k_salvage_scan<false>, sgrid, dim3(256), 0, st, a, s,
                           (const mcrc_dev::SalvageTile *)tiles, ntiles, tcnt, (const uint32_t *)nullptr,
                           (uint64_t *)nullptr, (uint32_t *)nullptr, (uint64_t)0);
        HIP_OK(hipEventRecord(d.ev1, st));
        scan32(st, tcnt, ntiles, tpre);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(h + mcrc_dev::kSvCand, s.ctr + mcrc_dev::kSvCand, 2 * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        (void)hipEventElapsedTime(&g_last_kernel_ms, d.ev0, d.ev1);  // (crc32c_last_kernel_ms: the scan's count pass)
        nc = h[mcrc_dev::kSvCand];
        work = h[mcrc_dev::kSvWork];
        return CRC32C_OK;
    }
    // (the item kernels index a batch in 32 bits: more candidates than that are past any honest buffer too)
    bool over() const { return mcrc::salvage_work_over(work, sc, a.region) || nc >= mcrc::kCountMax; }

    int candidates() {
        cand = d.sv_cand.reserve(nc * 8);
        cand_nt = d.sv_nt.reserve(nc * 4);
        cok = d.sv_ok.reserve(nc);
        if (!cand || !cand_nt || !cok) return CRC32C_ENOMEM;
        hipLaunchKernelGGL(mcrc_dev::k_salvage_scan<true>, sgrid, dim3(256), 0, st, a, s,
                           (const mcrc_dev::SalvageTile *)tiles, ntiles, (uint32_t *)nullptr, (const uint32_t *)tpre,
                           cand, cand_nt, nc);
        HIP_OK(hipGetLastError());
        mcrc_dev::SpanArgs v = a;
        v.offsets = cand;
        v.n = nc;
        v.ok = cok;
        Count count = nullptr;
        return run_items<1>(d, v, mcrc::item_route(nc, a.base_bytes, small_max()), st, &count);
    }

    // the count pass (cnt), the scan (into ppre) and, with out, the emit pass of
    // one of the pick's two kinds (SUSPECTS: shim_triage.h; sus: its arrays)
    template <bool SUSPECTS>
    void launch_pick(uint64_t *out, uint64_t ocap, const mcrc_dev::PickSuspects &sus) {
        auto launch = [&](auto kern, uint32_t *cnt, const uint32_t *pre, uint64_t *o, uint64_t cap) {
            hipLaunchKernelGGL(kern, pgrid, pblock, 0, st, (const uint64_t *)cand, (const uint32_t *)cand_nt,
                               (const uint8_t *)cok, nc, a.region, a.base_bytes, s.nw, cnt, pre, o, cap, sus);
        };
        launch(mcrc_dev::k_salvage_pick<false, SUSPECTS>, pcnt, nullptr, nullptr, 0);
        scan32(st, pcnt, s.nw, ppre);
        if (out) launch(mcrc_dev::k_salvage_pick<true, SUSPECTS>, nullptr, ppre, out, ocap);
    }

    // out (nullptr: counted only) takes the first ocap offsets found
    int pick(uint64_t *out, uint64_t ocap) {
        launch_pick<false>(out, ocap, mcrc_dev::PickSuspects{nullptr, nullptr, nullptr, nullptr});
        HIP_OK(hipGetLastError());
        return CRC32C_OK;
    }
};

// A host buffer is staged as the page walk stages it, host lists beside it,
// and the offsets found come back last.  (The per-piece scratch is the walk's
// own: its counts, scan and slots are free between calls.)
int salvage_pages(const void *base, uint64_t base_bytes, uint64_t wbuf_bytes, const uint64_t *walked,
                  const uint8_t *walked_ok, uint64_t nwalked, uint64_t *offsets, uint64_t cap, uint64_t *nfound,
                  uint64_t *scanned, uint64_t *ncand, unsigned flags, void *stream) {
    if (!base || !nfound || !wbuf_bytes || (cap && !offsets) || (nwalked && (!walked || !walked_ok)))
        return CRC32C_EINVAL;
    Device *dp = nullptr;
    int rc = current_device(&dp);
    if (rc) return rc;
    Device &d = *dp;
    hipStream_t st = (hipStream_t)stream;
    const bool dev = flags & CRC32C_DEVICE;
    if (dev && !device_range_ok(base, base_bytes)) return CRC32C_EINVAL;
    if (!dev)
        for (uint64_t i = 0; i < nwalked; ++i)
            if (walked[i] >= base_bytes || (i && walked[i - 1] >= walked[i])) return CRC32C_EINVAL;
    auto done = [&](uint64_t nf, uint64_t sc, uint64_t nc, int ret) {
        *nfound = nf;
        if (scanned) *scanned = sc;
        if (ncand) *ncand = nc;
        return ret;
    };
    const uint64_t nw = (base_bytes + wbuf_bytes - 1) / wbuf_bytes;
    if (nw == 0) return done(0, 0, 0, CRC32C_OK);
    if (nw >= 0x7fffffffull || nwalked >= mcrc::kCountMax) return CRC32C_EINVAL;
    std::lock_guard<std::mutex> lk(d.mu);
    Lease lease(d, st, !dev);  // (host: every exit drains st, the copies read and write the caller's memory)

    const uint8_t *dbase = (const uint8_t *)base;
    if (!dev) {
        uint8_t *b = d.stage.reserve(base_bytes);
        if (!b) return CRC32C_ENOMEM;
        HIP_OK(hipMemcpyAsync(b, base, base_bytes, hipMemcpyHostToDevice, st));
        dbase = b;
        if (nwalked) {
            uint64_t *lw = d.sv_walked.reserve(nwalked * 8);
            uint8_t *lo = d.sv_wok.reserve(nwalked);
            if (!lw || !lo) return CRC32C_ENOMEM;
            HIP_OK(hipMemcpyAsync(lw, walked, nwalked * 8, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(lo, walked_ok, nwalked, hipMemcpyHostToDevice, st));
            walked = lw;
            walked_ok = lo;
        }
    }
    SalvageRun r{d, st};
    if ((rc = r.init(item_args(d, dbase, base_bytes, wbuf_bytes, 0, flags), walked, walked_ok, nwalked, nw, d.walk_cnt,
                     d.walk_prefix, d.walk_slots)))
        return rc;
    if ((rc = r.regions(dev && nwalked))) return rc;
    if (r.ntiles == 0) return done(0, r.sc, 0, CRC32C_OK);
    if ((rc = r.scan())) return rc;
    if (r.nc == 0) return done(0, r.sc, 0, CRC32C_OK);
    if (r.over()) return done(0, r.sc, r.nc, CRC32C_EWORK);
    const bool direct = dev || cap == 0;  // (the caller's device array takes the offsets found)
    uint64_t *dout = direct ? offsets : d.sv_out.reserve(std::min(cap, r.nc) * 8);
    if (!direct && !dout) return CRC32C_ENOMEM;
    if ((rc = r.candidates())) return rc;
    if ((rc = r.pick(cap ? dout : nullptr, std::min(cap, r.nc)))) return rc;
    HIP_OK(hipMemcpyAsync(r.h32, r.ppre + nw, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const uint64_t nf = *r.h32, k = std::min(cap, nf);
    if (!direct && k) HIP_OK(hipMemcpy(offsets, dout, k * 8, hipMemcpyDeviceToHost));
    return done(nf, r.sc, r.nc, CRC32C_OK);
}

}  // namespace
