// shim_header.h -- repair_headers, the body of crc32c_repair_headers: the
// listed headers' candidate variants (k_header_variants, count and emit), the
// candidates' CRCs over the buffer as it stands through the span runners
// (run_spans: k_small or the planned path, chosen by span_route as for any
// batch; the spans may overlap) and the verdicts (k_header_apply), under one
// lock and one lease (k_header.h; the contract: include/crc32c_batch.h).  One
// read-back sizes the CRCs: the candidates and their spans' sum for the work
// bound, so a list with no candidates costs the variants kernel plus that
// read-back.  A host buffer is staged as crc32c_repair_items stages it,
// verdicts, positions and lengths come back through scratch, and the host
// inverts the accepted bits in the caller's buffer.
// Scratch (grow-only): per header 8 B of count and scan (a host call: 8 B of
// offset, 1 B of verdict, 8 B of position and 4 B of length more, and the
// staged buffer); per candidate 24 B (span offset, length, record, CRC).
#pragma once

namespace {

static_assert(mcrc::kHeaderBits == CRC32C_HEADER_BITS && mcrc::kHeaderWorkMax == CRC32C_HEADER_WORK_MAX,
              "header_geom.h restates the header's constants");
static_assert(mcrc::kHeaderVariants <= 64, "a lane of one wave per variant");
static_assert(mcrc::kHeaderListMax * mcrc::kHeaderVariants < mcrc::kCountMax, "the candidates' 32-bit scan is exact");

// The call's stages over a device-resident buffer and list (a.base, a.offsets,
// a.n = n >= 1), under a lock and a lease already held: repair_headers below
// and crc32c_scrub_pages (shim_scrub.h) call it.  The verdicts go to the device
// arrays d_ok, d_bit and d_lens; `keep`: nothing is written into the buffer.
// On CRC32C_OK the stream still runs: *counts (pinned) holds [kHdBad] and
// [kHdRepaired] once it has drained.  CRC32C_EWORK: the stream has drained and
// nothing was written.
int header_stages(Device &d, hipStream_t st, const mcrc_dev::SpanArgs &a, uint64_t base_bytes, uint64_t n,
                  uint8_t *d_ok, uint64_t *d_bit, uint32_t *d_lens, bool keep, unsigned long long **counts) {
    int rc;
    mcrc_dev::HeaderArgs h{};
    h.cnt = d.hd_cnt.reserve(n * 4);
    h.pre = d.hd_pre.reserve((n + 1) * 4);
    h.ctr = d.hd_ctr.reserve(mcrc_dev::kHdWords * sizeof(unsigned long long));
    unsigned long long *const hc = d.hd_host.reserve(mcrc_dev::kHdWords * sizeof(unsigned long long));
    if (!h.cnt || !h.pre || !h.ctr || !hc) return CRC32C_ENOMEM;
    *counts = hc;

    // the candidates counted, with their spans' sum for the work bound
    const dim3 grid((unsigned)std::min<uint64_t>((n + mcrc_dev::kHdWaves - 1) / mcrc_dev::kHdWaves,
                                                 (uint64_t)std::max(d.cus, 1) * 8)),
        block(64 * mcrc_dev::kHdWaves);
    HIP_OK(hipMemsetAsync(h.ctr, 0, mcrc_dev::kHdWords * sizeof(unsigned long long), st));
    HIP_OK(hipEventRecord(d.ev0, st));
    hipLaunchKernelGGL(mcrc_dev::k_header_variants<false>, grid, block, 0, st, a, h);
    HIP_OK(hipEventRecord(d.ev1, st));
    scan32(st, h.cnt, n, h.pre);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(hc, h.ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&g_last_kernel_ms, d.ev0, d.ev1);  // (crc32c_last_kernel_ms: the variants' count pass)
    const uint64_t work = hc[mcrc_dev::kHdWork], nc = hc[mcrc_dev::kHdCand];
    if (mcrc::header_work_over(work, base_bytes)) return CRC32C_EWORK;

    uint32_t *crc = nullptr;
    if (nc) {
        h.span_off = d.hd_off.reserve(nc * 8);
        h.span_len = d.hd_len.reserve(nc * 4);
        h.recs = d.hd_recs.reserve(nc * sizeof(mcrc_dev::HeaderRec));
        crc = d.hd_crc.reserve(nc * 4);
        if (!h.span_off || !h.span_len || !h.recs || !crc) return CRC32C_ENOMEM;
        h.ncap = nc;
        hipLaunchKernelGGL(mcrc_dev::k_header_variants<true>, grid, block, 0, st, a, h);
        HIP_OK(hipGetLastError());
        // their CRCs over the buffer as it stands (every span lies inside it: the variants are sane)
        crc32c_spans s{};
        s.base = a.base;
        s.base_bytes = base_bytes;
        s.offsets = h.span_off;
        s.lens = h.span_len;
        s.out = crc;
        s.n = nc;
        if ((rc = run_spans(d, s, mcrc::span_route(s, small_max()), st))) return rc;
    }
    hipLaunchKernelGGL(mcrc_dev::k_header_apply, grid, block, 0, st, a, h, (const uint32_t *)crc, d_ok, d_bit, d_lens,
                       (uint32_t)keep);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(hc + mcrc_dev::kHdBad, h.ctr + mcrc_dev::kHdBad, 2 * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st));
    return CRC32C_OK;
}

int repair_headers(void *base, uint64_t base_bytes, uint64_t region_bytes, const uint64_t *item_offsets, uint64_t n,
                   uint8_t *ok, uint64_t *bit, uint32_t *lens, uint64_t *nrepaired, uint64_t *nbad, unsigned flags,
                   void *stream) {
    if (!base || !item_offsets || !ok || !bit || !lens || !nrepaired || !nbad || n > mcrc::kHeaderListMax)
        return CRC32C_EINVAL;
    Device *dp = nullptr;
    int rc = current_device(&dp);
    if (rc) return rc;
    Device &d = *dp;
    *nrepaired = *nbad = 0;
    if (n == 0) {
        g_last_kernel_ms = 0.0f;
        return CRC32C_OK;
    }
    const bool dev = flags & CRC32C_DEVICE, locate_only = flags & CRC32C_LOCATE_ONLY;
    if (dev && !device_range_ok(base, base_bytes)) return CRC32C_EINVAL;
    std::lock_guard<std::mutex> lk(d.mu);
    hipStream_t st = dev ? (hipStream_t)stream : d.stream;  // (device: NULL is the default stream)
    if (!dev) HIP_OK(hipSetDevice(d.id));
    Lease lease(d, st, !dev);  // (host: every exit drains st, the copies read and write the caller's memory)

    mcrc_dev::SpanArgs a = item_args(d, base, base_bytes, region_bytes, n, flags);
    a.offsets = item_offsets;
    uint8_t *d_ok = ok;
    uint64_t *d_bit = bit;
    uint32_t *d_lens = lens;
    if (!dev) {
        uint8_t *b = d.stage.reserve(base_bytes);
        uint64_t *o = d.item_offs.reserve(n * 8);
        d_ok = d.hd_ok.reserve(n);
        d_bit = d.hd_bit.reserve(n * 8);
        d_lens = d.hd_lens.reserve(n * 4);
        if (!b || !o || !d_ok || !d_bit || !d_lens || !d.pin_ok.reserve(n) || !d.hd_hbit.reserve(n * 8) ||
            !d.hd_hlens.reserve(n * 4))
            return CRC32C_ENOMEM;
        HIP_OK(hipMemcpyAsync(b, base, base_bytes, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(o, item_offsets, n * 8, hipMemcpyHostToDevice, st));
        a.base = b;
        a.offsets = o;
    }
    // (a staged buffer is the call's own copy: the host inverts the caller's bits)
    unsigned long long *hc = nullptr;
    if ((rc = header_stages(d, st, a, base_bytes, n, d_ok, d_bit, d_lens, locate_only || !dev, &hc))) return rc;
    uint8_t *const h_ok = d.pin_ok.get();
    uint64_t *const h_bit = d.hd_hbit.get();
    uint32_t *const h_lens = d.hd_hlens.get();
    if (!dev) {
        HIP_OK(hipMemcpyAsync(h_ok, d_ok, n, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_bit, d_bit, n * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_lens, d_lens, n * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    if (!dev) {
        memcpy(ok, h_ok, n);
        memcpy(bit, h_bit, n * 8);
        memcpy(lens, h_lens, n * 4);
        if (!locate_only)
            for (uint64_t i = 0; i < n; ++i)
                if (ok[i] == CRC32C_ITEM_REPAIRED)
                    ((uint8_t *)base)[item_offsets[i] + bit[i] / 8] ^= (uint8_t)(1u << (bit[i] % 8));
    }
    *nbad = hc[mcrc_dev::kHdBad];
    *nrepaired = hc[mcrc_dev::kHdRepaired];
    return CRC32C_OK;
}

}  // namespace
