// shim_ptrs.h -- pointer batches (crc32c_batch_ptrs, crc32c_ptrs_submit,
// crc32c_chains_ptrs): a span's device address from the registry of
// page-locked ranges, the packed host pipeline (its plan is host_route.h's), the device
// batch behind k_ptr_rebase, and the chain fold both chain calls share.
#pragma once

namespace {

// The registry of page-locked ranges (mcrc::PinRegistry): crc32c_host_alloc and
// crc32c_host_register record, crc32c_host_free and crc32c_host_unregister
// forget.
mcrc::PinRegistry g_pin;

void pin_record(void *p, size_t bytes) {
    void *dv = nullptr;
    if (hipHostGetDevicePointer(&dv, p, 0) == hipSuccess) g_pin.record(p, bytes, dv);
    else (void)hipGetLastError();  // (not mapped: its spans are asked of the runtime, which refuses them too)
}
void pin_forget(void *p) { g_pin.forget(p); }

// The address a kernel reads the host span [p, p + len) at, or nullptr when it
// is not page-locked and mapped from end to end.  Memory page-locked by other
// means than the library's two calls is asked of the runtime, span by span.
const uint8_t *span_view(const void *p, uint64_t len) {
    const uint8_t *dv = nullptr;
    switch (g_pin.view(p, len, &dv)) {
        case mcrc::PinRegistry::Hit::inside: return dv;
        case mcrc::PinRegistry::Hit::cut: return nullptr;
        default: return device_view_range(p, len);
    }
}

// A long page-locked span is copied to its packed place by the copy engine, a
// short one by the host with the rest of its slot: a slot takes the DMA route
// when all its spans are page-locked and average this many bytes
// (profiles/ptr_batches.jsonl).
constexpr uint64_t kPtrDmaMin = 64u << 10;

// A host pointer batch through the pipeline's two slots, packed per
// mcrc::pack_chunk: slot c + 1 is packed (by the host, or by one DMA per span)
// and copied while slot c runs as an ordinary offsets batch over the slot;
// results come back in caller order.  views: each span's device view, or null
// when some span is pageable.
int run_ptr_host_batch(Device &d, const crc32c_ptr_batch &b, const uint8_t *const *views) {
    std::lock_guard<std::mutex> lk(d.mu);
    HIP_OK(hipSetDevice(d.id));
    int rc = ensure_slots(d, mcrc::kSlotBytes, mcrc::kSlotItems);
    if (rc) return rc;
    Lease lease(d, d.stream, true);  // (every exit waits for both streams, as in run_host_batch)
    d.acquire(d.copy);
    struct DrainCopy {
        hipStream_t copy;
        ~DrainCopy() { (void)hipStreamSynchronize(copy); }
    } drain_copy{d.copy};
    uint64_t pend_k0[2] = {0, 0}, pend_n[2] = {0, 0};  // results waiting in hout[slot]
    auto drain = [&](int k) -> int {
        if (!pend_n[k]) return CRC32C_OK;
        HIP_OK(hipEventSynchronize(d.done[k]));
        memcpy(b.out + pend_k0[k], d.hout[k].get(), pend_n[k] * 4);
        pend_n[k] = 0;
        return CRC32C_OK;
    };
    uint64_t k0 = 0;
    int slot = 0;
    while (k0 < b.n) {
        if ((rc = drain(slot))) return rc;  // slot free: its kernel and D2H are done
        uint64_t *const pos = d.hoffs[slot].get();
        const mcrc::PackChunk ch = mcrc::pack_chunk(b, k0, pos);
        const uint64_t cnt = ch.k1 - k0;
        if (!cnt) return CRC32C_EINVAL;  // (a span no slot takes: ptr_spans_ok refuses it first)
        uint8_t *const dbuf = d.dbuf[slot].get();
        if (views && cnt && ch.bytes / cnt >= kPtrDmaMin) {
            for (uint64_t k = k0; k < ch.k1; ++k)
                if (const uint64_t len = mcrc::ptr_len(b, k))
                    HIP_OK(hipMemcpyAsync(dbuf + pos[k - k0], b.ptrs[k], len, hipMemcpyHostToDevice, d.copy));
        } else if (ch.bytes) {
            mcrc::pack_copy(b, k0, ch.k1, pos, d.pin[slot].get());
            HIP_OK(hipMemcpyAsync(dbuf, d.pin[slot].get(), ch.bytes, hipMemcpyHostToDevice, d.copy));
        }
        uint32_t *const hlens = d.hlens[slot].get(), *const hcin = d.hcin[slot].get();
        if (b.lens) memcpy(hlens, b.lens + k0, cnt * 4);
        if (b.crc_in) memcpy(hcin, b.crc_in + k0, cnt * 4);
        crc32c_spans sub{};
        sub.base = dbuf;
        sub.base_bytes = ch.bytes;
        sub.offsets = d.doffs[slot].get();
        sub.lens = b.lens ? d.dlens[slot].get() : nullptr;
        sub.len = b.len;
        sub.crc_in = b.crc_in ? d.dcin[slot].get() : nullptr;
        sub.out = d.dout[slot].get();
        sub.n = cnt;
        HIP_OK(hipMemcpyAsync(d.doffs[slot].get(), pos, cnt * 8, hipMemcpyHostToDevice, d.copy));
        if (b.lens) HIP_OK(hipMemcpyAsync(d.dlens[slot].get(), hlens, cnt * 4, hipMemcpyHostToDevice, d.copy));
        if (b.crc_in) HIP_OK(hipMemcpyAsync(d.dcin[slot].get(), hcin, cnt * 4, hipMemcpyHostToDevice, d.copy));
        HIP_OK(hipEventRecord(d.copied[slot], d.copy));
        HIP_OK(hipStreamWaitEvent(d.stream, d.copied[slot], 0));
        // (the spans were packed by the host: none is out of range, nothing to count)
        const bool last = ch.k1 == b.n;  // the last slot's kernels are the ones timed
        if (last) HIP_OK(hipEventRecord(d.ev0, d.stream));
        if ((rc = run_spans(d, sub, mcrc::span_route(sub, small_max()), d.stream, nullptr, false,
                            last ? d.ev1 : nullptr)))
            return rc;
        HIP_OK(hipMemcpyAsync(d.hout[slot].get(), sub.out, cnt * 4, hipMemcpyDeviceToHost, d.stream));
        HIP_OK(hipEventRecord(d.done[slot], d.stream));
        pend_k0[slot] = k0;
        pend_n[slot] = cnt;
        k0 = ch.k1;
        slot ^= 1;
    }
    if ((rc = drain(slot)) || (rc = drain(slot ^ 1))) return rc;
    (void)hipEventElapsedTime(&g_last_kernel_ms, d.ev0, d.ev1);
    return CRC32C_OK;
}

// A CRC32C_DEVICE pointer batch on `st`.  Small by n and a fixed len: k_small
// over the pointers as absolute addresses.  Otherwise k_ptr_rebase's two
// launches and a 24-byte read-back make it the offsets batch {lo, hi - lo,
// scratch}, routed by the sum of its lengths.  device_range_ok is not applied:
// the extent spans allocations by design.
int device_ptr_batch(Device &d, const crc32c_ptr_batch &b, unsigned flags, hipStream_t st) {
    if (b.n == 0) return CRC32C_OK;
    const bool timed = !(flags & CRC32C_ASYNC);
    std::lock_guard<std::mutex> lk(d.mu);
    crc32c_spans s{};
    s.base_bytes = ~0ull;  // spans at absolute addresses
    s.offsets = (const uint64_t *)b.ptrs;
    s.lens = b.lens;
    s.len = b.len;
    s.crc_in = b.crc_in;
    s.out = b.out;
    s.n = b.n;
    // (what the host can tell before the rebase: lengths on the device count as too many bytes)
    mcrc::SpanRoute route = mcrc::SpanRoute::invalid;
    switch (mcrc::ptr_route(b.n, b.lens != nullptr, b.len, ~0ull, true, small_max())) {
        case mcrc::PtrRoute::invalid: return CRC32C_EINVAL;
        case mcrc::PtrRoute::small: route = mcrc::SpanRoute::small; break;
        default: break;
    }
    Count nrange = nullptr;
    {
        Lease lease(d, st);
        if (route != mcrc::SpanRoute::small) {
            uint64_t *const offs = d.ptr_offs.reserve(b.n * 8);
            unsigned long long *const red = d.ptr_red.reserve(24), *const hred = d.ptr_hred.reserve(24);
            if (!offs || !red || !hred) return CRC32C_ENOMEM;
            HIP_OK(hipMemsetAsync(red, 0xff, 8, st));
            HIP_OK(hipMemsetAsync(red + 1, 0, 16, st));
            const unsigned grid = (unsigned)std::min<uint64_t>(
                (b.n + mcrc_dev::kPtrThreads - 1) / mcrc_dev::kPtrThreads, 1024);
            for (uint32_t emit = 0; emit < 2; ++emit)
                hipLaunchKernelGGL(mcrc_dev::k_ptr_rebase, dim3(grid), dim3(mcrc_dev::kPtrThreads), 0, st,
                                   (const uint64_t *)b.ptrs, b.lens, b.len, b.n, red, offs, emit);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(hred, red, 24, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            const uint64_t lo = hred[0], hi = hred[1], sum = hred[2];
            const bool any = hi > lo;  // (no span with bytes: nothing is read, any mapped base will do)
            s.base = any ? (const void *)(uintptr_t)lo : (const void *)d.zero;
            s.base_bytes = any ? hi - lo : 0;
            s.offsets = offs;
            route = mcrc::ptr_span_route(s, sum, small_max());
        }
        if (timed) HIP_OK(hipEventRecord(d.ev0, st));
        const int rc = run_spans(d, s, route, st, timed ? &nrange : nullptr, true, timed ? d.ev1 : nullptr);
        if (rc || !timed) return rc;
    }
    HIP_OK(hipEventSynchronize(d.ev1));
    if (nrange) HIP_OK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&g_last_kernel_ms, d.ev0, d.ev1);
    return nrange && *nrange ? CRC32C_ERANGE : CRC32C_OK;
}

// The device views of a host pointer batch's spans (a span of no bytes: null,
// never used), or an empty vector when one of them is pageable.
std::vector<const uint8_t *> ptr_views(const crc32c_ptr_batch &b) {
    std::vector<const uint8_t *> v(b.n, nullptr);
    for (uint64_t i = 0; i < b.n; ++i)
        if (const uint64_t len = mcrc::ptr_len(b, i))
            if (!(v[i] = span_view(b.ptrs[i], len))) return {};
    return v;
}

// A host pointer batch that is not coalesced: packed, on the calling thread
// (or the dispatcher's).
int host_ptr_batch(Device &d, const crc32c_ptr_batch &b, const std::vector<const uint8_t *> &views) {
    return run_ptr_host_batch(d, b, views.empty() ? nullptr : views.data());
}

// A pointer job the dispatcher runs alone.
int run_ptr_job(Device &d, crc32c_job *j, hipStream_t st) {
    if (j->flags & CRC32C_DEVICE) return device_ptr_batch(d, j->pb, j->flags, st);
    return host_ptr_batch(d, j->pb, j->views);
}

// A new pointer job for the current device's queue: its spans translated now,
// coalescable when all of them are device-visible and short.
int make_ptr_job(const crc32c_ptr_batch &b, unsigned flags, crc32c_job **out) {
    if (b.n && (!b.ptrs || !b.out)) return CRC32C_EINVAL;
    Device *d = nullptr;
    int rc = current_device(&d);
    if (rc) return rc;
    Queue *q = nullptr;
    if ((rc = queue_of(*d, &q))) return rc;
    if (!(flags & CRC32C_DEVICE) && !mcrc::ptr_spans_ok(b)) return CRC32C_EINVAL;
    crc32c_job *j = new crc32c_job();
    j->ptr = true;
    j->pb = b;
    // (the fields the queue's launch and finish read of every job)
    j->s.lens = b.lens;
    j->s.len = b.len;
    j->s.crc_in = b.crc_in;
    j->s.out = b.out;
    j->s.n = b.n;
    j->flags = flags & ~(unsigned)CRC32C_ASYNC;
    j->q = q;
    if (flags & CRC32C_DEVICE) {
        if (hipEventCreateWithFlags(&j->after, hipEventDisableTiming) != hipSuccess ||
            hipEventRecord(j->after, nullptr) != hipSuccess) {
            if (j->after) (void)hipEventDestroy(j->after);
            delete j;
            return CRC32C_EHIP;
        }
    } else {
        j->views = ptr_views(b);
        bool short_spans = b.n >= 1 && b.n <= mcrc_dev::kSmallMax && !j->views.empty();
        for (uint64_t i = 0; short_spans && i < b.n; ++i) short_spans = mcrc::ptr_len(b, i) <= kQueueSpanMax;
        j->coalesce = short_spans;
    }
    *out = j;
    return CRC32C_OK;
}

int submit_or_free(crc32c_job *j) {
    if (j->q->submit(j)) return CRC32C_OK;
    if (j->after) (void)hipEventDestroy(j->after);
    delete j;
    return CRC32C_EHIP;
}

// crc32c_batch_ptrs.  Host: in place through the queue when the batch is
// coalescable and small by mcrc::ptr_route, else packed.
int batch_ptrs(const crc32c_ptr_batch &b, unsigned flags, hipStream_t stream) {
    if (b.n && (!b.ptrs || !b.out)) return CRC32C_EINVAL;
    Device *d = nullptr;
    int rc = current_device(&d);
    if (rc) return rc;
    if (b.n == 0) return CRC32C_OK;
    if (flags & CRC32C_DEVICE) return device_ptr_batch(*d, b, flags, stream);
    crc32c_job *j = nullptr;
    if ((rc = make_ptr_job(b, flags, &j))) return rc;
    uint64_t sum = 0;
    for (uint64_t i = 0; b.lens && i < b.n; ++i) sum += b.lens[i];
    const bool in_place =
        j->coalesce && mcrc::ptr_route(b.n, b.lens != nullptr, b.len, sum, true, small_max()) == mcrc::PtrRoute::small;
    if (!in_place) {
        rc = host_ptr_batch(*d, b, j->views);
        delete j;
        return rc;
    }
    if ((rc = submit_or_free(j))) return rc;
    rc = j->q->wait(j);
    delete j;
    return rc;
}

// The fold of crc32c_batch_chains and crc32c_chains_ptrs over the iovs' CRCs
// (crcs, lens / len: n of them, device memory for a device call) on st, with
// d.mu held: a host call's inputs are staged and `out` is filled when it
// returns; nrange: the iovs' out-of-range count, when one was taken.
int fold_chains(Device &d, const uint32_t *crcs, const uint32_t *lens, uint32_t len, uint64_t n,
                const uint64_t *chain_first, uint64_t nchains, uint32_t *out, bool dev, unsigned flags, hipStream_t st,
                Count nrange) {
    const uint64_t *first = chain_first;
    uint32_t *dout = out;
    if (!dev) {  // stage the fold's inputs
        uint8_t *buf = d.stage.reserve(mcrc::chain_stage_bytes(n, nchains));
        if (!buf) return CRC32C_ENOMEM;
        uint32_t *c_d = (uint32_t *)buf, *l_d = lens ? c_d + n : nullptr;
        uint64_t *f_d = (uint64_t *)(buf + mcrc::chain_first_off(n));
        HIP_OK(hipMemcpyAsync(c_d, crcs, n * 4, hipMemcpyHostToDevice, st));
        if (lens) HIP_OK(hipMemcpyAsync(l_d, lens, n * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(f_d, chain_first, (nchains + 1) * 8, hipMemcpyHostToDevice, st));
        crcs = c_d;
        lens = l_d;
        first = f_d;
        dout = (uint32_t *)(f_d + nchains + 1);
    }
    const int g = (int)std::min<uint64_t>((nchains + 255) / 256, 4096);
    hipLaunchKernelGGL(mcrc_dev::k_chain, dim3(g), dim3(256), 0, st, crcs, lens, len, first, nchains, dout,
                       (const uint32_t *)d.xpow);
    HIP_OK(hipGetLastError());
    if (!dev) HIP_OK(hipMemcpyAsync(out, dout, nchains * 4, hipMemcpyDeviceToHost, st));
    if (!dev || !(flags & CRC32C_ASYNC)) HIP_OK(hipStreamSynchronize(st));
    return nrange && *nrange ? CRC32C_ERANGE : CRC32C_OK;
}

bool host_chain_first_ok(const uint64_t *chain_first, uint64_t nchains, uint64_t n) {
    for (uint64_t c = 0; c < nchains; ++c)
        if (chain_first[c + 1] < chain_first[c] || chain_first[c + 1] > n) return false;
    return true;
}

// crc32c_chains_ptrs: the per-iov CRCs from the pointer path, then the fold.
// (A device call's iovs are waited for only with their own out-of-range count:
// an asynchronous call takes none.)
int chains_ptrs(const crc32c_ptr_batch &iovs, const uint64_t *chain_first, uint64_t nchains, uint32_t *out,
                unsigned flags, hipStream_t stream) {
    Device *d = nullptr;
    int rc = current_device(&d);
    if (rc) return rc;
    const bool dev = flags & CRC32C_DEVICE;
    if (!dev && !host_chain_first_ok(chain_first, nchains, iovs.n)) return CRC32C_EINVAL;
    rc = batch_ptrs(iovs, flags, stream);
    if (rc && rc != CRC32C_ERANGE) return rc;
    const bool range = rc == CRC32C_ERANGE;
    std::lock_guard<std::mutex> lk(d->mu);
    hipStream_t st = dev ? stream : d->stream;
    Lease lease(*d, st);
    rc = fold_chains(*d, iovs.out, iovs.lens, iovs.len, iovs.n, chain_first, nchains, out, dev, flags, st, nullptr);
    return rc ? rc : range ? CRC32C_ERANGE : CRC32C_OK;
}

}  // namespace
