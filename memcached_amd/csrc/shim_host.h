// shim_host.h -- the host pipeline (run_host_batch; its order and chunk cuts
// are host_route.h's) and item_images, the body of crc32c_verify_items and
// crc32c_stamp_items.
#pragma once

namespace {

int ensure_slots(Device &d, uint64_t bytes, uint64_t items) {
    for (int k = 0; k < 2; ++k)
        if (!d.dbuf[k].reserve(bytes) || !d.pin[k].reserve(bytes) || !d.doffs[k].reserve(items * 8) ||
            !d.dlens[k].reserve(items * 4) || !d.dcin[k].reserve(items * 4) || !d.dout[k].reserve(items * 4) ||
            !d.hoffs[k].reserve(items * 8) || !d.hlens[k].reserve(items * 4) || !d.hcin[k].reserve(items * 4) ||
            !d.hout[k].reserve(items * 4))
            return CRC32C_ENOMEM;
    return CRC32C_OK;
}

// Host-resident batch on one device.  Spans are staged in offset order
// (mcrc::staging_order) in chunks (mcrc::next_chunk) that go through two
// pipeline slots: while chunk c is checksummed, chunk c+1 is staged into
// pinned memory (unless the caller's buffer is already pinned) and copied H2D
// on the copy stream.  Descriptors and results travel through pinned twins so
// no copy touches pageable memory; results are scattered back to the caller's
// order.
int run_host_batch(Device &d, const crc32c_spans &s) {
    std::lock_guard<std::mutex> lk(d.mu);
    HIP_OK(hipSetDevice(d.id));
    if (s.n == 0) return CRC32C_OK;
    if (!mcrc::host_spans_ok(s)) return CRC32C_EINVAL;
    const std::vector<uint64_t> order = mcrc::staging_order(s);  // staging position -> caller index
    auto idx = [&](uint64_t k) { return order.empty() ? k : order[k]; };
    int rc = ensure_slots(d, mcrc::kSlotBytes, mcrc::kSlotItems);
    if (rc) return rc;
    // Every exit waits for both streams (an H2D copy may still be reading the
    // caller's pinned buffer after an error): the copy stream first, then the
    // lease drains the library stream and hands the scratch on.
    Lease lease(d, d.stream, true);
    d.acquire(d.copy);
    struct DrainCopy {
        hipStream_t copy;
        ~DrainCopy() { (void)hipStreamSynchronize(copy); }
    } drain_copy{d.copy};
    const bool src_pinned = is_pinned_or_device(s.base, s.base_bytes);
    const uint8_t *src = (const uint8_t *)s.base;
    uint64_t pend_k0[2] = {0, 0}, pend_n[2] = {0, 0};  // results waiting in hout[slot]
    auto drain = [&](int k) -> int {
        if (!pend_n[k]) return CRC32C_OK;
        HIP_OK(hipEventSynchronize(d.done[k]));
        const uint32_t *hout = d.hout[k].get();
        if (order.empty()) memcpy(s.out + pend_k0[k], hout, pend_n[k] * 4);
        else
            for (uint64_t i = 0; i < pend_n[k]; ++i) s.out[order[pend_k0[k] + i]] = hout[i];
        pend_n[k] = 0;
        return CRC32C_OK;
    };
    uint64_t k0 = 0;
    int slot = 0;
    while (k0 < s.n) {
        const mcrc::Chunk ch = mcrc::next_chunk(s, order, k0);
        const uint64_t lo = ch.lo, bytes = ch.hi - lo, cnt = ch.k1 - k0;
        if ((rc = drain(slot))) return rc;  // slot free: its kernel and D2H are done
        const uint8_t *h2d_src = src + lo;
        if (!src_pinned) {
            memcpy(d.pin[slot].get(), src + lo, bytes);
            h2d_src = d.pin[slot].get();
        }
        uint64_t *const hoffs = d.hoffs[slot].get();
        uint32_t *const hlens = d.hlens[slot].get(), *const hcin = d.hcin[slot].get();
        for (uint64_t i = 0; i < cnt; ++i) {
            const uint64_t c = idx(k0 + i);
            hoffs[i] = mcrc::span_off(s, c) - lo;
            if (s.lens) hlens[i] = s.lens[c];
            if (s.crc_in) hcin[i] = s.crc_in[c];
        }
        crc32c_spans sub{};
        sub.base = d.dbuf[slot].get();
        sub.base_bytes = bytes;
        sub.offsets = d.doffs[slot].get();
        sub.lens = s.lens ? d.dlens[slot].get() : nullptr;
        sub.len = s.len;
        sub.crc_in = s.crc_in ? d.dcin[slot].get() : nullptr;
        sub.out = d.dout[slot].get();
        sub.n = cnt;
        HIP_OK(hipMemcpyAsync(d.dbuf[slot].get(), h2d_src, bytes, hipMemcpyHostToDevice, d.copy));
        HIP_OK(hipMemcpyAsync(d.doffs[slot].get(), hoffs, cnt * 8, hipMemcpyHostToDevice, d.copy));
        if (s.lens) HIP_OK(hipMemcpyAsync(d.dlens[slot].get(), hlens, cnt * 4, hipMemcpyHostToDevice, d.copy));
        if (s.crc_in) HIP_OK(hipMemcpyAsync(d.dcin[slot].get(), hcin, cnt * 4, hipMemcpyHostToDevice, d.copy));
        HIP_OK(hipEventRecord(d.copied[slot], d.copy));
        HIP_OK(hipStreamWaitEvent(d.stream, d.copied[slot], 0));
        // (the spans were checked on the host: nothing to count)
        if ((rc = run_spans(d, sub, mcrc::span_route(sub, small_max()), d.stream))) return rc;
        HIP_OK(hipMemcpyAsync(d.hout[slot].get(), sub.out, cnt * 4, hipMemcpyDeviceToHost, d.stream));
        HIP_OK(hipEventRecord(d.done[slot], d.stream));
        pend_k0[slot] = k0;
        pend_n[slot] = cnt;
        k0 = ch.k1;
        slot ^= 1;
    }
    if ((rc = drain(slot)) || (rc = drain(slot ^ 1))) return rc;
    return CRC32C_OK;
}

// The CRCs a host stamp call got back, written into the caller's images
// (exptime, bytes 28..31: storage.c:567).
void scatter_stamps(void *base, const uint64_t *offs, const uint8_t *ok, const uint32_t *crc, uint64_t n) {
    uint8_t *bb = (uint8_t *)base;
    for (uint64_t i = 0; i < n; ++i)
        if (ok[i] == CRC32C_ITEM_STAMPED) memcpy(bb + offs[i] + 28, &crc[i], 4);
}

template <class F>  // f(std::integral_constant<int, MODE>): MODE 2, or 3 under CRC32C_KEEP_STAMPED
int with_stamp_mode(unsigned flags, F f) {
    return (flags & CRC32C_KEEP_STAMPED) ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 2>{});
}

// Item-image batches (MODE 1 verify, 2 stamp, 3 stamp with CRC32C_KEEP_STAMPED)
// over a packed buffer of item images at item_offsets.
//   device: in place on the caller's stream;
//   host, small (at most 8 MiB, a wbuf or an IO batch): one k_small launch on
//     the library stream that reads the images where they are when the buffer
//     is page-locked (crc32c_host_alloc / _register; stamps are written into
//     it in place), else from a pinned copy; descriptors and results through
//     pinned mapped scratch -- no device allocation, no copy engine;
//   host, large: staged into grow-only device scratch, planned kernels.
template <int MODE>
int item_images(void *base, uint64_t base_bytes, uint64_t region_bytes, const uint64_t *item_offsets, uint64_t n,
                uint8_t *ok, uint64_t *nbad, unsigned flags, void *stream) {
    if (!base || !item_offsets || (MODE == 1 && !ok)) return CRC32C_EINVAL;
    Device *d = nullptr;
    int rc = current_device(&d);
    if (rc) return rc;
    if (n == 0) {
        if (nbad) *nbad = 0;
        return CRC32C_OK;
    }
    const bool dev = flags & CRC32C_DEVICE;
    if (dev && !device_range_ok(base, base_bytes)) return CRC32C_EINVAL;
    mcrc_dev::SpanArgs a = item_args(*d, base, base_bytes, region_bytes, n, flags);
    a.offsets = item_offsets;
    // (past the small batches: K5 or the planned path for device images, the planned path for staged ones)
    const mcrc::ItemRoute route = mcrc::item_route(n, base_bytes, small_max(), dev);
    Count count = nullptr;
    std::lock_guard<std::mutex> lk(d->mu);
    if (dev) {
        hipStream_t st = (hipStream_t)stream;  // NULL: the default stream
        a.ok = ok;
        a.out = nullptr;  // stamp: write into the images
        {
            Lease lease(*d, st);
            if ((rc = run_items<MODE>(*d, a, route, st, &count))) return rc;
        }
        if ((flags & CRC32C_ASYNC) && !nbad) return CRC32C_OK;  // fire and forget
        HIP_OK(hipStreamSynchronize(st));
        if (nbad) *nbad = *count;
        return CRC32C_OK;
    }
    hipStream_t st = d->stream;
    HIP_OK(hipSetDevice(d->id));
    Lease lease(*d, st, true);  // (every exit drains st first: the kernels write pinned scratch)
    const bool small = route == mcrc::ItemRoute::small;
    uint64_t *const h_offs = d->pin_offs.reserve(n * 8);
    uint8_t *const h_ok = d->pin_ok.reserve(n);
    if (!h_offs || !h_ok) return CRC32C_ENOMEM;
    memcpy(h_offs, item_offsets, n * 8);
    const uint8_t *mapped = device_view_range(base, base_bytes);
    // stamp results come back as CRCs (scattered into the caller's images
    // here) unless the kernel stamps the caller's page-locked buffer itself
    const bool crcs_back = MODE >= 2 && !(small && mapped);
    const uint32_t *const h_crc = crcs_back ? d->pin_crc.reserve(n * 4) : nullptr;
    if (crcs_back && !h_crc) return CRC32C_ENOMEM;
    a.ok = d->pin_ok.dev();
    a.out = crcs_back ? d->pin_crc.dev() : nullptr;
    if (small) {
        if (!mapped) {  // a pinned copy the kernel reads
            uint8_t *const h_stage = d->pin_stage.reserve(base_bytes);
            if (!h_stage) return CRC32C_ENOMEM;
            memcpy(h_stage, base, base_bytes);
            mapped = d->pin_stage.dev();
        }
        a.base = mapped;
        a.offsets = d->pin_offs.dev();
    } else {
        uint8_t *b = d->stage.reserve(base_bytes);
        uint64_t *o = d->item_offs.reserve(n * 8);
        uint8_t *r = d->item_out.reserve(n * 5 + 4);  // ok[n], then (4-B aligned) crc[n]
        if (!b || !o || !r) return CRC32C_ENOMEM;
        HIP_OK(hipMemcpyAsync(b, base, base_bytes, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(o, h_offs, n * 8, hipMemcpyHostToDevice, st));
        a.base = b;
        a.offsets = o;
        a.ok = r;
        a.out = crcs_back ? (uint32_t *)(r + ((n + 3) & ~3ull)) : nullptr;
    }
    if ((rc = run_items<MODE>(*d, a, route, st, &count))) return rc;
    if (!small) {  // the staged batch's results
        HIP_OK(hipMemcpyAsync(h_ok, a.ok, n, hipMemcpyDeviceToHost, st));
        if (crcs_back) HIP_OK(hipMemcpyAsync(d->pin_crc.get(), a.out, n * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    if (crcs_back) scatter_stamps(base, item_offsets, h_ok, h_crc, n);
    if (ok) memcpy(ok, h_ok, n);
    if (nbad) *nbad = *count;
    return CRC32C_OK;
}

}  // namespace
