// shim_salvage.h -- salvage_pages, the body of crc32c_salvage_pages: the
// regions from the walk's lists, the scan of the eligible bytes, the
// candidates' CRCs through the item runners, the pick (k_salvage.h; the
// contract: include/crc32c_batch.h).
#pragma once

namespace {

static_assert(mcrc::kSalvageWorkMax == CRC32C_SALVAGE_WORK_MAX, "the work bound's factor is the header's");

// Three counts are read back, each once: the tiles (what the scan's scratch is
// sized by; a list that fails its check ends the call here), the candidates and
// their work (none, or past the bound, ends it there; else they size the
// verify), and the images found.  A host buffer is staged as the page walk
// stages it, host lists beside it, and the offsets found come back last.
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

    mcrc_dev::SalvageArgs s{};
    const uint8_t *dbase = (const uint8_t *)base;
    s.walked = walked;
    s.walked_ok = walked_ok;
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
            s.walked = lw;
            s.walked_ok = lo;
        }
    }
    unsigned long long *h = d.sv_host.reserve(8 * sizeof(unsigned long long));  // the counters' pinned twin + a count
    uint32_t *h32 = (uint32_t *)(h + mcrc_dev::kSvWords);
    // (the walk's own scratch: its counts, scan and slots are free between calls)
    uint32_t *pcnt = d.walk_cnt.reserve((2 * nw + 2) * 4), *ppre = d.walk_prefix.reserve((nw + 2) * 4);
    s.slots = d.walk_slots.reserve((size_t)nw * mcrc_dev::kSvSlots * 16);
    s.nregs = pcnt ? pcnt + nw + 1 : nullptr;
    s.ctr = d.sv_ctr.reserve(mcrc_dev::kSvWords * sizeof(unsigned long long));
    if (!h || !pcnt || !ppre || !s.ctr || !s.slots) return CRC32C_ENOMEM;
    s.nwalked = nwalked;
    s.nw = nw;
    s.ba = (uint32_t)((uintptr_t)dbase & (mcrc::kSalvageTile - 1));
    mcrc_dev::SpanArgs a = item_args(d, dbase, base_bytes, wbuf_bytes, 0, flags);
    const dim3 pgrid(mcrc::walk_grid(nw)), pblock(64 * mcrc_dev::kWalkWaves);

    // the regions, counted
    HIP_OK(hipMemsetAsync(s.ctr, 0, mcrc_dev::kSvWords * sizeof(unsigned long long), st));
    if (dev && nwalked)
        hipLaunchKernelGGL(mcrc_dev::k_salvage_check, dim3(mcrc::final_grid(nwalked)), dim3(256), 0, st, s, base_bytes);
    hipLaunchKernelGGL(mcrc_dev::k_salvage_regions<false>, pgrid, pblock, 0, st, a, s, pcnt, (const uint32_t *)nullptr,
                       (mcrc_dev::SalvageTile *)nullptr, (uint64_t)0);
    hipLaunchKernelGGL(mcrc_dev::k_scan32, dim3(1), dim3(1024), 0, st, (const uint32_t *)pcnt, nw, ppre);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h, s.ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h32, ppre + nw, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (h[mcrc_dev::kSvBad]) return CRC32C_EINVAL;
    const uint64_t sc = h[mcrc_dev::kSvScanned];
    const uint32_t ntiles = *h32;
    g_last_kernel_ms = 0.0f;  // (no scan ran yet: not the time of an earlier call)
    if (ntiles == 0) return done(0, sc, 0, CRC32C_OK);

    // the scan, counted
    mcrc_dev::SalvageTile *tiles = d.sv_tiles.reserve((size_t)ntiles * sizeof(mcrc_dev::SalvageTile));
    uint32_t *tcnt = d.sv_tcnt.reserve((size_t)ntiles * 4), *tpre = d.sv_tpre.reserve(((size_t)ntiles + 1) * 4);
    if (!tiles || !tcnt || !tpre) return CRC32C_ENOMEM;
    hipLaunchKernelGGL(mcrc_dev::k_salvage_regions<true>, pgrid, pblock, 0, st, a, s, (uint32_t *)nullptr,
                       (const uint32_t *)ppre, tiles, (uint64_t)ntiles);
    const dim3 sgrid((unsigned)std::min<uint64_t>(((uint64_t)ntiles + 3) / 4, (uint64_t)std::max(d.cus, 1) * 8));
    HIP_OK(hipEventRecord(d.ev0, st));
    hipLaunchKernelGGL(mcrc_dev::k_salvage_scan<false>, sgrid, dim3(256), 0, st, a, s,
                       (const mcrc_dev::SalvageTile *)tiles, ntiles, tcnt, (const uint32_t *)nullptr,
                       (uint64_t *)nullptr, (uint32_t *)nullptr, (uint64_t)0);
    HIP_OK(hipEventRecord(d.ev1, st));
    hipLaunchKernelGGL(mcrc_dev::k_scan32, dim3(1), dim3(1024), 0, st, (const uint32_t *)tcnt, (uint64_t)ntiles, tpre);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h + mcrc_dev::kSvCand, s.ctr + mcrc_dev::kSvCand, 2 * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&g_last_kernel_ms, d.ev0, d.ev1);  // (crc32c_last_kernel_ms: the scan's count pass)
    const uint64_t nc = h[mcrc_dev::kSvCand], work = h[mcrc_dev::kSvWork];
    if (nc == 0) return done(0, sc, 0, CRC32C_OK);
    // (the item kernels index a batch in 32 bits: more candidates than that are past any honest buffer too)
    if (mcrc::salvage_work_over(work, sc, wbuf_bytes) || nc >= mcrc::kCountMax) return done(0, sc, nc, CRC32C_EWORK);

    // the candidates, their CRCs, the pick
    uint64_t *cand = d.sv_cand.reserve(nc * 8);
    uint32_t *cand_nt = d.sv_nt.reserve(nc * 4);
    uint8_t *cok = d.sv_ok.reserve(nc);
    const bool direct = dev || cap == 0;  // (the caller's device array takes the offsets found)
    uint64_t *dout = direct ? offsets : d.sv_out.reserve(std::min(cap, nc) * 8);
    if (!cand || !cand_nt || !cok || (!direct && !dout)) return CRC32C_ENOMEM;
    hipLaunchKernelGGL(mcrc_dev::k_salvage_scan<true>, sgrid, dim3(256), 0, st, a, s,
                       (const mcrc_dev::SalvageTile *)tiles, ntiles, (uint32_t *)nullptr, (const uint32_t *)tpre, cand,
                       cand_nt, nc);
    HIP_OK(hipGetLastError());
    a.offsets = cand;
    a.n = nc;
    a.ok = cok;
    Count count = nullptr;
    if ((rc = run_items<1>(d, a, mcrc::item_route(nc, base_bytes, small_max()), st, &count))) return rc;
    auto pick = [&](auto kern, uint32_t *cnt, const uint32_t *pre, uint64_t *out, uint64_t ocap) {
        hipLaunchKernelGGL(kern, pgrid, pblock, 0, st, (const uint64_t *)cand, (const uint32_t *)cand_nt,
                           (const uint8_t *)cok, nc, wbuf_bytes, base_bytes, nw, cnt, pre, out, ocap);
    };
    pick(mcrc_dev::k_salvage_pick<false>, pcnt, nullptr, nullptr, 0);
    hipLaunchKernelGGL(mcrc_dev::k_scan32, dim3(1), dim3(1024), 0, st, (const uint32_t *)pcnt, nw, ppre);
    if (cap) pick(mcrc_dev::k_salvage_pick<true>, nullptr, ppre, dout, std::min(cap, nc));
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h32, ppre + nw, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const uint64_t nf = *h32, k = std::min(cap, nf);
    if (!direct && k) HIP_OK(hipMemcpy(offsets, dout, k * 8, hipMemcpyDeviceToHost));
    return done(nf, sc, nc, CRC32C_OK);
}

}  // namespace
