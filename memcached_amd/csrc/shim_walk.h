// shim_walk.h -- the page walk: walk_count (the count pass: k_walk<false>, the
// scan, the total read back), walk_items (the emit pass and the items' verify
// or stamp) and walk_pages, the body of crc32c_verify_pages and
// crc32c_stamp_pages.
#pragma once

namespace {

int walk_count(Device &d, hipStream_t st, const void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t nw,
               unsigned flags, mcrc_dev::SpanArgs *a, mcrc_dev::WalkOut *out, uint32_t *total) {
    const uint8_t *dbase = (const uint8_t *)base;
    if (!(flags & CRC32C_DEVICE)) {
        uint8_t *b = d.stage.reserve(base_bytes);
        if (!b) return CRC32C_ENOMEM;
        HIP_OK(hipMemcpyAsync(b, base, base_bytes, hipMemcpyHostToDevice, st));
        dbase = b;
    }
    // counts of nw wbufs and a zero: the exclusive scan's last entry is the total
    uint32_t *cnt = d.walk_cnt.reserve((nw + 1) * 4);
    uint32_t *prefix = d.walk_prefix.reserve((nw + 2) * 4);
    if (!cnt || !prefix) return CRC32C_ENOMEM;
    *a = item_args(d, dbase, base_bytes, wbuf_bytes, 0, flags);
    mcrc_dev::WalkOut &wo = *out;
    wo = mcrc_dev::WalkOut{};
    wo.cnt = cnt;
    wo.prefix = prefix;
    // (no slots kept either when their buffer cannot be allocated)
    wo.kslot = mcrc::walk_kslot(wbuf_bytes);
    wo.slots = wo.kslot ? d.walk_slots.reserve((size_t)nw * wo.kslot * 8) : nullptr;
    if (!wo.slots) wo.kslot = 0;
    HIP_OK(hipMemsetAsync(cnt + nw, 0, 4, st));
    hipLaunchKernelGGL(mcrc_dev::k_walk<false>, dim3(mcrc::walk_grid(nw)), dim3(64 * mcrc_dev::kWalkWaves), 0, st, *a,
                       nw, wo);
    scan32(st, cnt, nw + 1, prefix);
    HIP_OK(hipMemcpyAsync(total, prefix + nw, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return CRC32C_OK;
}

// The walk's second half, enqueued on st behind walk_count: the emit pass and
// the verify or stamp of the `total` items it lists.  The emit pass writes the
// items' offsets into doffs: copied from the count pass's slots, or for a wbuf
// of more items than those (or with no slots kept) by walking it again.  A
// planned verify then reads the headers in k_count; only with no slots kept
// does the second walk write its plan entries too.  dcrc: a host stamp's CRCs
// (nullptr: a stamp writes into the images).
template <int MODE>
int walk_items(Device &d, hipStream_t st, mcrc_dev::SpanArgs a, mcrc_dev::WalkOut wo, uint64_t nw, uint64_t total,
               uint64_t *doffs, uint8_t *dok, uint32_t *dcrc, Count *count) {
    a.offsets = wo.offs = doffs;
    a.n = total;
    a.ok = dok;
    a.out = dcrc;
    const mcrc::ItemRoute route = mcrc::item_route(total, a.base_bytes, small_max(), !dcrc);
    const bool counted = MODE < 2 && route == mcrc::ItemRoute::planned && wo.kslot == 0;
    if (counted) {
        const int rc = ensure_plan(d, total, mcrc::plan_cap(total, a.base_bytes));
        if (rc) return rc;
        a.span_acc = d.span_acc.get();
        wo.nunit = d.nunit.get();
        wo.irec = d.irec.get();
        wo.fast = d.fast.get();
    }
    return run_items<MODE>(d, a, route, st, count, &wo, nw, counted);
}

// crc32c_verify_pages (MODE 1) and crc32c_stamp_pages (MODE 2 / 3).  cap == 0
// is a count-only query for a verify; a stamp still stamps (a device one then
// computes no ok flags).  A host verify copies the first cap results into the
// caller's arrays; a host stamp runs on the staged copy, every offset, flag
// and CRC comes back through pinned scratch and the stamps are scattered into
// the caller's buffer here (`scatter`: its lease drains the stream on every exit).
template <int MODE>
int walk_pages(void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t *offsets, uint8_t *ok, uint64_t cap,
               uint64_t *nitems, uint64_t *nbad, unsigned flags, void *stream) {
    constexpr bool kStamp = MODE >= 2;
    if (!base || !wbuf_bytes || !nitems || !nbad || (cap && (!offsets || !ok))) return CRC32C_EINVAL;
    Device *dp = nullptr;
    int rc = current_device(&dp);
    if (rc) return rc;
    Device &d = *dp;
    hipStream_t st = (hipStream_t)stream;
    const bool dev = flags & CRC32C_DEVICE;
    if (dev && !device_range_ok(base, base_bytes)) return CRC32C_EINVAL;
    std::lock_guard<std::mutex> lk(d.mu);
    const uint64_t nw = (base_bytes + wbuf_bytes - 1) / wbuf_bytes;
    const bool scatter = kStamp && !dev;
    Lease lease(d, st, scatter);
    *nitems = *nbad = 0;
    if (nw == 0 || nw >= 0x7fffffffull) return nw ? CRC32C_EINVAL : CRC32C_OK;
    mcrc_dev::SpanArgs a;
    mcrc_dev::WalkOut wo;
    uint32_t found = 0;
    if ((rc = walk_count(d, st, base, base_bytes, wbuf_bytes, nw, flags, &a, &wo, &found))) return rc;
    const uint64_t total = found, k = std::min<uint64_t>(cap, total);
    *nitems = total;
    if (total == 0 || (!kStamp && cap == 0)) return CRC32C_OK;
    // the caller's device arrays take the results when every item fits, else
    // walk scratch (a device call that wants no per-item output: no ok flags)
    const bool direct = dev && cap >= total, want_ok = !dev || cap;
    uint64_t *doffs = direct ? offsets : d.walk_offs.reserve((size_t)total * 8), *h_offs = nullptr;
    uint8_t *dok = direct ? ok : want_ok ? d.walk_ok.reserve(total) : nullptr, *h_ok = nullptr;
    uint32_t *dcrc = nullptr, *h_crc = nullptr;
    if (!doffs || (!dok && want_ok)) return CRC32C_ENOMEM;
    if (scatter) {
        dcrc = (uint32_t *)d.item_out.reserve((size_t)total * 4);
        h_offs = d.pin_offs.reserve(total * 8);
        h_ok = d.pin_ok.reserve(total);
        h_crc = d.pin_crc.reserve(total * 4);
        if (!dcrc || !h_offs || !h_ok || !h_crc) return CRC32C_ENOMEM;
    }
    Count count = nullptr;
    if ((rc = walk_items<MODE>(d, st, a, wo, nw, total, doffs, dok, dcrc, &count))) return rc;
    if (scatter) {
        HIP_OK(hipMemcpyAsync(h_offs, doffs, total * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_ok, dok, total, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_crc, dcrc, total * 4, hipMemcpyDeviceToHost, st));
    } else if (!direct && k) {
        const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        HIP_OK(hipMemcpyAsync(offsets, doffs, k * 8, kind, st));
        HIP_OK(hipMemcpyAsync(ok, dok, k, kind, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    *nbad = count[0];
    if (count[1]) return CRC32C_EWALK;
    if (scatter) {
        scatter_stamps(base, h_offs, h_ok, h_crc, total);
        if (k) {
            memcpy(offsets, h_offs, k * 8);
            memcpy(ok, h_ok, k);
        }
    }
    return CRC32C_OK;
}

}  // namespace
