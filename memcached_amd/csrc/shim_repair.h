// shim_repair.h -- repair_items, the body of crc32c_repair_items: the images'
// CRCs through the item runners (run_items<2> with the CRCs sent to scratch:
// k_small or the planned path, the routes that honour SpanArgs::out), the
// listing of the images whose stored CRC differs, the search for the bit that
// explains each difference and the verdicts (k_repair.h; the contract:
// include/crc32c_batch.h), under one lock and one lease.  One read-back sizes
// the search: the listed images, their chunks and their spans' sum for the work
// bound, so a clean list costs the CRCs plus one count.  A host buffer is
// staged as crc32c_verify_items stages a large one, verdicts and positions come
// back through scratch, and the host inverts the accepted bits in the caller's
// buffer.  crc32c_repair_bytes (repair_bytes below) is the same runner under
// the byte rule: the search and apply kernels of k_repair_bytes.h, a mask
// array beside the positions, and the host XORs masks where it inverted bits.
// Scratch (grow-only): per image 4 B of CRC, 8 B of counts and 8 B of their
// scans (a host call: 8 B of offset, 1 B of verdict and 8 B of position more,
// and the staged buffer); per listed image a 24-B record, 4 B of first chunk
// and 4 B of located position.
#pragma once

namespace {

static_assert(mcrc_dev::kItemRepaired == CRC32C_ITEM_REPAIRED, "the verdict the kernels write is the header's");
static_assert(mcrc::kRepairSpanMax == CRC32C_REPAIR_SPAN_MAX && mcrc::kRepairSpanDefault == CRC32C_REPAIR_SPAN_DEFAULT &&
                  mcrc::kRepairNoBit == CRC32C_NO_BIT,
              "repair_geom.h restates the header's constants");
static_assert(32 + 8 * (uint64_t)CRC32C_REPAIR_SPAN_MAX < mcrc::kRepairOrder, "a located position is unique");
static_assert(mcrc::kRepairBytesSpanMax == CRC32C_REPAIR_BYTES_SPAN_MAX &&
                  mcrc::kRepairBytesSpanDefault == CRC32C_REPAIR_BYTES_SPAN_DEFAULT,
              "repair_geom.h restates the header's constants");

// The call's stages over a device-resident buffer and list (a.base, a.offsets,
// a.n = n >= 1, route: item_route's for them), under a lock and a lease already
// held: repair_items below and crc32c_scrub_pages (shim_scrub.h) call it.  The
// verdicts go to the device arrays d_ok and d_bit; `keep`: nothing is written
// into the buffer.  On CRC32C_OK the stream still runs: *counts (pinned) holds
// [kRpBad] and [kRpRepaired] once it has drained, and with *searched the
// search's time lies between ev0 and ev1.  CRC32C_EWORK: the stream has
// drained and nothing was written.
// d_mask: crc32c_repair_bytes' rule -- max_span is then the resolved one, d_bit
// takes the located bytes and d_mask their masks (k_repair_bytes.h).
int item_stages(Device &d, hipStream_t st, const mcrc_dev::SpanArgs &a, uint64_t base_bytes, uint64_t n,
                mcrc::ItemRoute route, uint32_t max_span, uint8_t *d_ok, uint64_t *d_bit, bool keep,
                unsigned long long **counts, bool *searched, uint8_t *d_mask = nullptr) {
    int rc;
    mcrc_dev::RepairArgs r{};
    r.max_span = max_span ? max_span : CRC32C_REPAIR_SPAN_DEFAULT;
    r.ok = d_ok;
    r.bit = d_bit;
    uint32_t *const crc = d.rp_crc.reserve(n * 4);
    r.lcnt = d.rp_lcnt.reserve(n * 4);
    r.ccnt = d.rp_ccnt.reserve(n * 4);
    uint32_t *const lpre = d.rp_lpre.reserve((n + 1) * 4), *const cpre = d.rp_cpre.reserve((n + 1) * 4);
    r.ctr = d.rp_ctr.reserve(mcrc_dev::kRpWords * sizeof(unsigned long long));
    unsigned long long *const h = d.rp_host.reserve((mcrc_dev::kRpWords + 1) * sizeof(unsigned long long));
    if (!crc || !r.lcnt || !r.ccnt || !lpre || !cpre || !r.ctr || !h) return CRC32C_ENOMEM;
    r.crc = crc;
    *counts = h;
    *searched = false;
    uint32_t *const h32 = (uint32_t *)(h + mcrc_dev::kRpWords);  // the two scans' totals

    if (d_mask) HIP_OK(hipMemsetAsync(d_mask, 0, n, st));  // (k_repair_count leaves it alone)

    // the images' CRCs, into scratch
    mcrc_dev::SpanArgs c = a;
    c.out = crc;
    c.ok = nullptr;
    Count count = nullptr;
    if ((rc = run_items<2>(d, c, route, st, &count))) return rc;

    // the verdicts that need no search, the listed images and the work bound's sum
    const unsigned grid = (unsigned)mcrc::count_grid(n);
    HIP_OK(hipMemsetAsync(r.ctr, 0, mcrc_dev::kRpWords * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(mcrc_dev::k_repair_count, dim3(grid), dim3(256), 0, st, a, r);
    scan32(st, r.lcnt, n, lpre);
    scan32(st, r.ccnt, n, cpre);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h, r.ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h32, lpre + n, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h32 + 1, cpre + n, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    g_last_kernel_ms = 0.0f;  // (no search ran yet: not the time of an earlier call)
    const uint64_t nl = h32[0], work = h[mcrc_dev::kRpWork];
    // (the chunks' 32-bit sum is exact below the bound: a chunk per kRepairChunk bytes of span and one per image)
    if (work > base_bytes || work / mcrc::kRepairChunk + 2 * nl >= mcrc::kCountMax) return CRC32C_EWORK;
    const uint64_t nchunks = h32[1];

    if (nl) {
        mcrc_dev::RepairRec *const recs = d.rp_recs.reserve(nl * sizeof(mcrc_dev::RepairRec));
        uint32_t *const first = d.rp_first.reserve(nl * 4), *const found = d.rp_found.reserve(nl * 4);
        if (!recs || !first || !found) return CRC32C_ENOMEM;
        hipLaunchKernelGGL(mcrc_dev::k_repair_emit, dim3(grid), dim3(256), 0, st, a, r, (const uint32_t *)lpre,
                           (const uint32_t *)cpre, recs, first, found, nl);
        // a lane per chunk, eight workgroups per CU at the most
        const uint64_t sgrid = std::min<uint64_t>((nchunks + 255) / 256, (uint64_t)std::max(d.cus, 1) * 8);
        HIP_OK(hipEventRecord(d.ev0, st));
        hipLaunchKernelGGL(d_mask ? mcrc_dev::k_repair_bytes_search : mcrc_dev::k_repair_search,
                           dim3((unsigned)sgrid), dim3(256), 0, st, (const mcrc_dev::RepairRec *)recs,
                           (const uint32_t *)first, nl, nchunks, (const uint32_t *)d.xpow, found);
        HIP_OK(hipEventRecord(d.ev1, st));
        const dim3 agrid((unsigned)mcrc::final_grid(nl));
        if (d_mask)
            hipLaunchKernelGGL(mcrc_dev::k_repair_bytes_apply, agrid, dim3(256), 0, st, a, r, d_mask,
                               (const mcrc_dev::RepairRec *)recs, (const uint32_t *)found, nl, (uint32_t)keep);
        else
            hipLaunchKernelGGL(mcrc_dev::k_repair_apply, agrid, dim3(256), 0, st, a, r,
                               (const mcrc_dev::RepairRec *)recs, (const uint32_t *)found, nl, (uint32_t)keep);
        HIP_OK(hipGetLastError());
        *searched = true;
    }
    HIP_OK(hipMemcpyAsync(h + mcrc_dev::kRpBad, r.ctr + mcrc_dev::kRpBad, 2 * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st));
    return CRC32C_OK;
}

// The runner of crc32c_repair_items (mask == nullptr: bit[] takes bit indices)
// and of crc32c_repair_bytes (bit[] takes byte indices, mask[] their masks;
// max_span: the resolved one).  The argument checks are the callers'.
int repair_run(void *base, uint64_t base_bytes, uint64_t region_bytes, const uint64_t *item_offsets, uint64_t n,
               uint32_t max_span, uint8_t *ok, uint64_t *bit, uint8_t *mask, uint64_t *nrepaired, uint64_t *nbad,
               unsigned flags, void *stream) {
    Device *dp = nullptr;
    int rc = current_device(&dp);
    if (rc) return rc;
    Device &d = *dp;
    *nrepaired = *nbad = 0;
    if (n == 0) return CRC32C_OK;
    const bool dev = flags & CRC32C_DEVICE, locate_only = flags & CRC32C_LOCATE_ONLY;
    if (dev && !device_range_ok(base, base_bytes)) return CRC32C_EINVAL;
    // (k_small, or the planned path: K5's stamps go into the images themselves)
    const mcrc::ItemRoute route = mcrc::item_route(n, base_bytes, small_max(), false);
    if (route == mcrc::ItemRoute::invalid) return CRC32C_EINVAL;
    std::lock_guard<std::mutex> lk(d.mu);
    hipStream_t st = dev ? (hipStream_t)stream : d.stream;  // (device: NULL is the default stream)
    if (!dev) HIP_OK(hipSetDevice(d.id));
    Lease lease(d, st, !dev);  // (host: every exit drains st, the copies read and write the caller's memory)

    mcrc_dev::SpanArgs a = item_args(d, base, base_bytes, region_bytes, n, flags);
    a.offsets = item_offsets;
    uint8_t *d_ok = ok, *d_mask = mask;
    uint64_t *d_bit = bit;
    if (!dev) {
        uint8_t *b = d.stage.reserve(base_bytes);
        uint64_t *o = d.item_offs.reserve(n * 8);
        d_ok = d.rp_ok.reserve(n);
        d_bit = d.rp_bit.reserve(n * 8);
        if (mask) d_mask = d.rp_mask.reserve(n);
        if (!b || !o || !d_ok || !d_bit || !d.pin_ok.reserve(n) || !d.rp_hbit.reserve(n * 8) ||
            (mask && (!d_mask || !d.rp_hmask.reserve(n))))
            return CRC32C_ENOMEM;
        HIP_OK(hipMemcpyAsync(b, base, base_bytes, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(o, item_offsets, n * 8, hipMemcpyHostToDevice, st));
        a.base = b;
        a.offsets = o;
    }
    // (a staged buffer is the call's own copy: the host inverts the caller's bits)
    unsigned long long *h = nullptr;
    bool searched = false;
    if ((rc = item_stages(d, st, a, base_bytes, n, route, max_span, d_ok, d_bit, locate_only || !dev, &h, &searched,
                          d_mask)))
        return rc;
    uint8_t *const h_ok = d.pin_ok.get(), *const h_mask = d.rp_hmask.get();
    uint64_t *const h_bit = d.rp_hbit.get();
    if (!dev) {
        HIP_OK(hipMemcpyAsync(h_ok, d_ok, n, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_bit, d_bit, n * 8, hipMemcpyDeviceToHost, st));
        if (mask) HIP_OK(hipMemcpyAsync(h_mask, d_mask, n, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    if (searched) (void)hipEventElapsedTime(&g_last_kernel_ms, d.ev0, d.ev1);  // (crc32c_last_kernel_ms: the search)
    if (!dev) {
        memcpy(ok, h_ok, n);
        memcpy(bit, h_bit, n * 8);
        if (mask) memcpy(mask, h_mask, n);
        if (!locate_only)
            for (uint64_t i = 0; i < n; ++i)
                if (ok[i] == CRC32C_ITEM_REPAIRED) {
                    if (mask) ((uint8_t *)base)[item_offsets[i] + bit[i]] ^= mask[i];
                    else ((uint8_t *)base)[item_offsets[i] + bit[i] / 8] ^= (uint8_t)(1u << (bit[i] % 8));
                }
    }
    *nbad = h[mcrc_dev::kRpBad];
    *nrepaired = h[mcrc_dev::kRpRepaired];
    return CRC32C_OK;
}

int repair_items(void *base, uint64_t base_bytes, uint64_t region_bytes, const uint64_t *item_offsets, uint64_t n,
                 uint32_t max_span, uint8_t *ok, uint64_t *bit, uint64_t *nrepaired, uint64_t *nbad, unsigned flags,
                 void *stream) {
    if (!base || !item_offsets || !ok || !bit || !nrepaired || !nbad || max_span > CRC32C_REPAIR_SPAN_MAX)
        return CRC32C_EINVAL;
    return repair_run(base, base_bytes, region_bytes, item_offsets, n, max_span, ok, bit, nullptr, nrepaired, nbad,
                      flags, stream);
}

// crc32c_repair_bytes: the same runner under the byte rule.  Nothing of `out`
// is written before the device is known (CRC32C_ENODEV leaves it alone).
int repair_bytes(void *base, uint64_t base_bytes, uint64_t region_bytes, const uint64_t *item_offsets, uint64_t n,
                 const crc32c_bytes_opts *opts, crc32c_bytes_out *out) {
    static const crc32c_bytes_opts none{};
    const crc32c_bytes_opts &op = opts ? *opts : none;
    if (!base || !item_offsets || !out || !out->ok || !out->byte || !out->mask ||
        op.max_span > CRC32C_REPAIR_BYTES_SPAN_MAX)
        return CRC32C_EINVAL;
    const unsigned flags = op.mode & (unsigned)(CRC32C_DEVICE | CRC32C_CFLAGS64 | CRC32C_LOCATE_ONLY);
    return repair_run(base, base_bytes, region_bytes, item_offsets, n,
                      op.max_span ? op.max_span : CRC32C_REPAIR_BYTES_SPAN_DEFAULT, out->ok, out->byte, out->mask,
                      &out->nrepaired, &out->nbad, flags, op.stream);
}

}  // namespace
