// shim_launch.h -- one launch function per route and the runners (run_spans,
// run_items, run_copy) that enqueue a routed batch and own its bad count.
// Routes and grid sizes come from host_route.h.
#pragma once

namespace {

thread_local float g_last_kernel_ms = -1.0f;

std::atomic<uint64_t> g_small_max{mcrc_dev::kSmallMax};  // crc32c_set_small_max
uint64_t small_max() { return g_small_max.load(std::memory_order_relaxed); }
std::atomic<uint64_t> g_k1_tail_min{mcrc_dev::kK1TailMinSteps};  // crc32c_set_k1_tail_min

// out[0..n] = the exclusive scan of in[0..n) and its total: the step between a
// count pass and its emit pass (one workgroup).
void scan32(hipStream_t st, const uint32_t *in, uint64_t n, uint32_t *out) {
    hipLaunchKernelGGL(mcrc_dev::k_scan32, dim3(1), dim3(1024), 0, st, in, n, out);
}

int ensure_plan(Device &d, uint64_t n, uint64_t cap) {
    const uint64_t ntiles = mcrc::plan_tiles(n);
    // (one more unit record per share boundary)
    const uint64_t shares = (uint64_t)mcrc::kMaxRounds * mcrc::span_groups(d.cus);
    const bool ok = d.nunit.reserve(n * 8) && d.tile_sum.reserve(ntiles * sizeof(mcrc_dev::PlanSum)) &&
                    d.tile_pre.reserve((ntiles + 1) * sizeof(mcrc_dev::PlanSum)) &&
                    d.whole.reserve(n * sizeof(mcrc_dev::UnitRec)) && d.irec.reserve(n * sizeof(uint4)) &&
                    d.span_acc.reserve(n * 4) && d.big.reserve(n * sizeof(uint4)) && d.fast.reserve(n) &&
                    d.fastidx.reserve(n * 4) && d.units.reserve((cap + shares) * sizeof(mcrc_dev::UnitRec)) &&
                    d.counters.reserve(16) && d.starts.reserve((shares + 1) * 4);
    return ok ? CRC32C_OK : CRC32C_ENOMEM;
}

// The fields every batch shares: the device's tables and the counter of bad
// or out-of-range spans (the device's shared one, or the coalescing queue's
// own); 4-B client flags unless the caller says otherwise.
mcrc_dev::SpanArgs common_args(const Device &d, unsigned long long *nbad = nullptr) {
    mcrc_dev::SpanArgs a{};
    a.nbad = nbad ? nbad : d.nbad;
    a.segpow = d.segpow;
    a.xpow = d.xpow;
    a.tab8 = d.tab8;
    a.zero = d.zero;
    a.cfl = 4;
    return a;
}

mcrc_dev::SpanArgs span_args(const Device &d, const crc32c_spans &s) {
    mcrc_dev::SpanArgs a = common_args(d);
    a.base = (const uint8_t *)s.base;
    a.base_bytes = s.base_bytes;
    a.offsets = s.offsets;
    a.stride = s.stride;
    a.lens = s.lens;
    a.len = s.len;
    a.crc_in = s.crc_in;
    a.out = s.out;
    a.n = s.n;
    return a;
}

// An item-image batch: n images at a.offsets of [base, base + base_bytes).
mcrc_dev::SpanArgs item_args(const Device &d, const void *base, uint64_t base_bytes, uint64_t region_bytes, uint64_t n,
                             unsigned flags) {
    mcrc_dev::SpanArgs a = common_args(d);
    a.base = (const uint8_t *)base;
    a.base_bytes = base_bytes;
    a.n = n;
    a.region = region_bytes;
    a.cfl = (flags & CRC32C_CFLAGS64) ? 8u : 4u;
    return a;
}

// The counters of a K1 launch of n items on st, or null: the launch is then
// split evenly.  Null below the tail's threshold, for a stream without a slot
// (k1_slots.h) and for a capturing stream: a replayed graph may run twice at
// once, on one slot.
mcrc_dev::K1Ctl *k1_ctl(const Device &d, uint64_t n, hipStream_t st) {
    const uint64_t waves = (uint64_t)mcrc::grid_for(d.cus, n) * (1024 / 64);
    const uint64_t cg = ((n + 1) / 2 + waves - 1) / waves;
    if (cg < g_k1_tail_min.load(std::memory_order_relaxed)) return nullptr;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (cap != hipStreamCaptureStatusNone) return nullptr;
    const int slot = d.k1_slots.find((void *)st, (void *)hipStreamLegacy, (void *)hipStreamPerThread);
    return slot < 0 ? nullptr : d.k1_ctl + slot;
}

// K1.  Non-temporal loads only when every 128-B line belongs to one item.
int launch_k1(const Device &d, const crc32c_spans &s, hipStream_t st) {
    const bool nt = ((uintptr_t)s.base & 127u) == 0 && (s.stride & 127u) == 0;
    mcrc_dev::K1Ctl *ctl = k1_ctl(d, s.n, st);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(mcrc::grid_for(d.cus, s.n)), dim3(1024), mcrc_dev::kLdsImageK1Bytes, st,
                           (const uint8_t *)s.base, s.stride, s.n, (const uint4 *)d.img, (const uint32_t *)s.crc_in,
                           s.out, ctl);
    };
    if (s.crc_in) nt ? go(mcrc_dev::k_fixed<true, true>) : go(mcrc_dev::k_fixed<true, false>);
    else nt ? go(mcrc_dev::k_fixed<false, true>) : go(mcrc_dev::k_fixed<false, false>);
    HIP_OK(hipGetLastError());
    return CRC32C_OK;
}

// K5's kernel for a batch of n spans or images.
template <int MODE, bool OFFS>
void launch_k5(const Device &d, const mcrc_dev::SpanArgs &a, mcrc_dev::ItemsOut io, hipStream_t st) {
    const int grid = mcrc::grid_for(d.cus, a.n);
    io.xm128 = d.xm128;
    io.nsr = mcrc::k5_nsr(grid, a.n);
    hipLaunchKernelGGL((mcrc_dev::k_lines<MODE, OFFS>), dim3(grid), dim3(1024), mcrc_dev::kLdsImageK1Bytes, st, a,
                       d.img, io);
}

// k_small over a's spans on st, a workgroup per `per` of them (counters as the
// caller set them in a).
template <int MODE>
int launch_small(const Device &d, const mcrc_dev::SpanArgs &a, hipStream_t st) {
    const uint64_t per = mcrc::small_per(d.cus, a.n);
    hipLaunchKernelGGL((mcrc_dev::k_small<MODE>), dim3((unsigned)((a.n + per - 1) / per)), dim3((unsigned)(32 * per)),
                       mcrc_dev::kLdsImageK1Bytes, st, a, d.img);
    HIP_OK(hipGetLastError());
    return CRC32C_OK;
}

void launch_spans(const Device &d, const mcrc_dev::SpanArgs &x, int grid, hipStream_t st) {
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(mcrc_dev::kSpanBlock), mcrc_dev::kLdsImageK1Bytes, st, x, d.img);
    };
    x.units ? go(mcrc_dev::k_spans<true>) : go(mcrc_dev::k_spans<false>);
}

// The fixed-length routes that need no plan: K5, or k_blocks / k_spans / neither and k_final.
int launch_fixed(const Device &d, const mcrc_dev::SpanArgs &a, hipStream_t st, mcrc::SpanRoute route) {
    using R = mcrc::SpanRoute;
    const int grid = mcrc::grid_for(d.cus, a.n);
    if (route == R::k5) {
        mcrc_dev::ItemsOut io{};  // (MODE 0: K5 stores every CRC itself)
        a.offsets ? launch_k5<0, true>(d, a, io, st) : launch_k5<0, false>(d, a, io, st);
        HIP_OK(hipGetLastError());
        return CRC32C_OK;
    }
    auto blocks = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(1024), mcrc_dev::kLdsImageK1Bytes, st, a, d.img,
                           (const uint4 *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr);
    };
    if (route == R::id_blocks)
        a.offsets ? blocks(mcrc_dev::k_blocks<true, true>) : blocks(mcrc_dev::k_blocks<true, false>);
    else if (route == R::id_spans)
        launch_spans(d, a, grid, st);
    hipLaunchKernelGGL((mcrc_dev::k_final<0, false>), dim3(mcrc::final_grid(a.n)), dim3(256), 0, st, a, nullptr);
    HIP_OK(hipGetLastError());
    return CRC32C_OK;
}

// The planned path.  counted: the page walk's second pass wrote k_count's entries.
template <int MODE>
int launch_planned(Device &d, mcrc_dev::SpanArgs a, hipStream_t st, bool counted) {
    const uint64_t n = a.n;
    const uint64_t cap = mcrc::plan_cap(n, a.base_bytes);
    int rc = ensure_plan(d, n, cap);
    if (rc) return rc;
    uint32_t *nvalid = d.counters.get(), *nwhole = nvalid + 1, *nbig = nvalid + 2;
    uint64_t *const nunit = d.nunit.get();
    uint4 *const irec = d.irec.get();
    uint8_t *const fast = d.fast.get();
    uint32_t *const starts = d.starts.get();
    mcrc_dev::UnitRec *const units = d.units.get();
    HIP_OK(hipMemsetAsync(nvalid, 0, 12, st));  // nvalid, nwhole, nbig
    // the balanced plan's shares: rounds x the span kernel's groups
    const uint32_t rounds = mcrc::plan_rounds(a.base_bytes);
    const uint32_t shares = rounds * mcrc::span_groups(d.cus);
    HIP_OK(hipMemsetAsync(starts, 0xff, ((uint64_t)shares + 1) * 4, st));
    a.span_acc = d.span_acc.get();
    if (!counted)
        hipLaunchKernelGGL((mcrc_dev::k_count<MODE>), dim3(mcrc::count_grid(n)), dim3(256), 0, st, a, nunit, irec,
                           fast);
    // prefix sums of the plan (units, blocks, one-block spans): tile sums, one
    // workgroup over them, then each tile rescanned where k_expand uses it
    const uint64_t ntiles = mcrc::plan_tiles(n);
    const int gt = mcrc::plan_tile_grid(n);
    // (a.dn: n is the list's upper bound and its length is read on the device)
    mcrc_dev::PlanSum *const tile_pre = d.tile_pre.get(), *const total = tile_pre + ntiles;
    hipLaunchKernelGGL(mcrc_dev::k_plan_tiles, dim3(gt), dim3(mcrc_dev::kPlanThreads), 0, st, (const uint64_t *)nunit,
                       (const uint8_t *)fast, n, a.dn, d.tile_sum.get());
    hipLaunchKernelGGL(mcrc_dev::k_plan_scan, dim3(1), dim3(mcrc_dev::kPlanThreads), 0, st,
                       (const mcrc_dev::PlanSum *)d.tile_sum.get(), n, a.dn, tile_pre, total);
    const uint32_t *nfast = &total->fast;
    hipLaunchKernelGGL(mcrc_dev::k_expand, dim3(gt), dim3(mcrc_dev::kPlanThreads), 0, st, a.base, (const uint64_t *)nunit,
                       (const uint8_t *)fast, (const mcrc_dev::PlanSum *)tile_pre, (const mcrc_dev::PlanSum *)total,
                       (const uint4 *)irec, n, a.dn, units, cap, nvalid, d.whole.get(), nwhole, d.big.get(), nbig,
                       d.fastidx.get(), shares, starts);
    hipLaunchKernelGGL(mcrc_dev::k_expand_big, dim3(1024), dim3(256), 0, st, a.base, (const uint64_t *)nunit,
                       (const mcrc_dev::PlanSum *)total, (const uint4 *)irec, units, (const uint4 *)d.big.get(),
                       (const uint32_t *)nbig, n, a.dn, shares, starts);
    mcrc_dev::SpanArgs u = a;
    u.units = units;
    u.nunits = nvalid;
    u.segpow = d.segpow;
    u.starts = starts;
    u.rounds = rounds;
    // spans whose unit is one whole block: k_blocks over the compacted list;
    // the other spans' units: the span kernel
    hipLaunchKernelGGL((mcrc_dev::k_blocks<false, true>), dim3(mcrc::grid_for(d.cus, n)), dim3(1024),
                       mcrc_dev::kLdsImageK1Bytes, st, u, d.img, (const uint4 *)irec, (const uint32_t *)d.fastidx.get(),
                       (const uint32_t *)nfast);
    launch_spans(d, u, d.cus, st);
    mcrc_dev::SpanArgs w = u;  // (every table pointer set, even those whole units do not use)
    w.units = d.whole.get();
    w.nunits = nwhole;
    w.starts = nullptr;
    launch_spans(d, w, d.cus, st);
    hipLaunchKernelGGL((mcrc_dev::k_final<MODE, true>), dim3(mcrc::final_grid(n)), dim3(256), 0, st, u, irec);
    HIP_OK(hipGetLastError());
    return CRC32C_OK;
}

// K5 over the item images of a (MODE 1 verify, MODE 2 stamp, MODE 3 stamp that
// keeps carried CRCs; device memory): k_census routes the batch on the device,
// k_lines checksums the one-block images (+ k_fix for stamps) and lists the
// others, and the planned path takes that list with its length read on the
// device (a.dn).  Nothing is read back: an async stamp stays async.
template <int MODE>
int launch_items(Device &d, mcrc_dev::SpanArgs a, hipStream_t st) {
    const uint64_t n = a.n;
    mcrc_dev::ItemsOut io{};
    io.fb = d.fb.reserve(n * 4);
    io.nfb = d.nfb;
    io.route = d.route;
    constexpr bool kStamp = MODE >= 2;
    if (kStamp) io.rt = d.rt.reserve(n * 8);
    uint64_t *fo = d.fb_offs.reserve(n * 8);
    uint8_t *fok = d.fb_ok.reserve(n);
    if (!io.fb || (kStamp && !io.rt) || !fo || !fok) return CRC32C_ENOMEM;
    HIP_OK(hipMemsetAsync(d.nfb, 0, 4, st));
    hipLaunchKernelGGL(mcrc_dev::k_census<MODE>, dim3(1), dim3(mcrc_dev::kCensus), 0, st, a, d.route);
    launch_k5<MODE, true>(d, a, io, st);
    const unsigned g = (unsigned)mcrc::final_grid(n);
    // Once k_fix is forked, every exit joins it back into st, error exits
    // included: the caller's busy event (recorded on st after this returns)
    // must cover k_fix's writes to the images and its reads of io.rt.
    struct Join {
        hipStream_t st;
        hipEvent_t ev;
        bool armed = false;
        ~Join() {
            if (armed) (void)hipStreamWaitEvent(st, ev, 0);
        }
    } join{st, d.join};
    if (kStamp) {
        // k_fix (the stamps of the images k_lines checksummed) on the side
        // stream, beside the planned path of the images it listed: its
        // scattered partial-sector writes and that path's small launches
        // overlap.  They touch disjoint bytes unless images overlap
        // (crc32c_batch.h: then an image's CRC may or may not see another
        // image's new stamp).
        HIP_OK(hipEventRecord(d.fork, st));
        HIP_OK(hipStreamWaitEvent(d.side, d.fork, 0));
        hipLaunchKernelGGL(mcrc_dev::k_fix, dim3(g), dim3(256), 0, d.side, a, (const uint2 *)io.rt,
                           (const uint32_t *)d.route, d.xm128);
        HIP_OK(hipEventRecord(d.join, d.side));
        join.armed = true;
    }
    hipLaunchKernelGGL(mcrc_dev::k_gather_offs, dim3(g), dim3(256), 0, st, a.offsets, (const uint32_t *)io.fb,
                       (const uint32_t *)d.nfb, fo, (const uint32_t *)d.route);
    HIP_OK(hipGetLastError());
    mcrc_dev::SpanArgs f = a;
    const bool want_ok = MODE == 1 || a.ok;
    f.offsets = fo;
    f.dn = d.nfb;  // (f.n = n: the list's upper bound)
    f.ok = want_ok ? fok : nullptr;
    int rc = launch_planned<MODE>(d, f, st, false);
    if (kStamp) {
        join.armed = false;
        HIP_OK(hipStreamWaitEvent(st, d.join, 0));  // (also when the planned path failed)
    }
    if (rc) return rc;
    if (want_ok)
        hipLaunchKernelGGL(mcrc_dev::k_scatter_ok, dim3(g), dim3(256), 0, st, (const uint8_t *)fok,
                           (const uint32_t *)io.fb, (const uint32_t *)d.nfb, a.ok, (const uint32_t *)d.route);
    HIP_OK(hipGetLastError());
    return CRC32C_OK;
}

// The bad count of a batch is delivered as a pointer to pinned host words,
// valid once the stream has drained (nullptr: not delivered): count[0] bad
// images or spans out of range; count[1], for a walk, its failed self-checks
// (CRC32C_EWALK) and, for a copy, the sane images that did not fit dst.
typedef const unsigned long long *Count;

// Own count (where a runner says so; elsewhere k_small adds to the shared
// counter like every kernel): k_small or k_copy counts in words of its own,
// zero between calls, and its last workgroup hands the count to d.hbad.
void count_own(const Device &d, mcrc_dev::SpanArgs *a) {
    a->nbad = d.small_nbad;
    a->host_nbad = d.hbad;
    a->done = d.small_done;
}
// Shared count: the kernels add to d.nbad[0..words) (common_args; [1]: the
// walk's), zeroed by the runner before them and copied to d.hbad after them.
int count_copy(const Device &d, int words, hipStream_t st, Count *count) {
    HIP_OK(hipMemcpyAsync(d.hbad, d.nbad, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    *count = d.hbad;
    return CRC32C_OK;
}

// Enqueue a routed span batch on st.  count (nullptr: the caller does not take
// it) is delivered for spans given by offsets or lengths, the only ones that
// can be out of range: zeroed, counted and copied, or the small route's own
// count with own_small.  mark: recorded after the kernels.  K1 needs no d.mu.
int run_spans(Device &d, const crc32c_spans &s, mcrc::SpanRoute route, hipStream_t st, Count *count = nullptr,
              bool own_small = false, hipEvent_t mark = nullptr) {
    using R = mcrc::SpanRoute;
    if (route == R::invalid) return CRC32C_EINVAL;
    const bool checked = count && (s.offsets || s.lens);
    bool copy = false;
    int rc = CRC32C_OK;
    if (route == R::k1) {
        rc = launch_k1(d, s, st);
    } else if (route != R::empty) {
        mcrc_dev::SpanArgs a = span_args(d, s);
        if (route == R::small && count && own_small) {
            count_own(d, &a);
            if (checked) *count = d.hbad;
        } else {
            HIP_OK(hipMemsetAsync(d.nbad, 0, sizeof(unsigned long long), st));
            copy = checked;
        }
        rc = route == R::small     ? launch_small<0>(d, a, st)
             : route == R::planned ? launch_planned<0>(d, a, st, false)
                                   : launch_fixed(d, a, st, route);
    }
    if (rc) return rc;
    if (mark) HIP_OK(hipEventRecord(mark, st));
    return copy ? count_copy(d, 1, st, count) : CRC32C_OK;
}

// Enqueue a routed item-image batch on st; the count is always delivered (own
// count on the small route).  walk: the emit pass of a page walk over nw wbufs
// (shim_walk.h) runs first, behind one memset of both shared counters, and
// count[1] delivers its self-check; counted: it writes k_count's entries.
template <int MODE>
int run_items(Device &d, mcrc_dev::SpanArgs a, mcrc::ItemRoute route, hipStream_t st, Count *count,
              const mcrc_dev::WalkOut *walk = nullptr, uint64_t nw = 0, bool counted = false) {
    using R = mcrc::ItemRoute;
    if (route == R::invalid) return CRC32C_EINVAL;
    const int words = walk ? 2 : 1;
    const bool own = route == R::small && !walk;
    if (own) {
        count_own(d, &a);
        *count = d.hbad;
    } else {
        HIP_OK(hipMemsetAsync(d.nbad, 0, words * sizeof(unsigned long long), st));
    }
    if (walk) {
        mcrc_dev::WalkOut wo = *walk;
        wo.err = d.nbad + 1;
        hipLaunchKernelGGL(mcrc_dev::k_walk<true>, dim3(mcrc::walk_grid(nw)), dim3(64 * mcrc_dev::kWalkWaves), 0, st, a,
                           nw, wo);
        HIP_OK(hipGetLastError());
    }
    const int rc = route == R::small ? launch_small<MODE>(d, a, st)
                   : route == R::k5  ? launch_items<MODE>(d, a, st)
                                     : launch_planned<MODE>(d, a, st, counted);
    if (rc) return rc;
    return own ? CRC32C_OK : count_copy(d, words, st, count);
}

// Enqueue k_copy over a's images on st: at most a workgroup per CU (past one
// image per group the groups stride over the list).  Own count, count[1] too.
int run_copy(const Device &d, mcrc_dev::SpanArgs a, mcrc_dev::CopyArgs ca, hipStream_t st, Count *count) {
    const uint64_t per = mcrc::small_per(d.cus, a.n);
    const uint64_t grid = std::min<uint64_t>((a.n + per - 1) / per, (uint64_t)std::max(d.cus, 1));
    count_own(d, &a);
    ca.nrange = d.small_done + 1;
    *count = d.hbad;
    hipLaunchKernelGGL(mcrc_dev::k_copy, dim3((unsigned)grid), dim3((unsigned)(32 * per)), mcrc_dev::kLdsImageK1Bytes,
                       st, a, ca, d.img);
    HIP_OK(hipGetLastError());
    return CRC32C_OK;
}

// The body of crc32c_batch for CRC32C_DEVICE on `st`: a synchronous batch
// records the kernel time; ERANGE when a span lay outside the buffer.
int device_batch(Device &d, const crc32c_spans &s, unsigned flags, hipStream_t st) {
    if (s.n && !device_range_ok(s.base, s.base_bytes)) return CRC32C_EINVAL;
    const mcrc::SpanRoute route = mcrc::span_route(s, small_max());
    const bool timed = !(flags & CRC32C_ASYNC);
    // an asynchronous K1 batch needs nothing the lock guards (no scratch, no
    // timing events): IO or device threads enqueue it concurrently
    if (!timed && route == mcrc::SpanRoute::k1) return run_spans(d, s, route, st);
    std::lock_guard<std::mutex> lk(d.mu);
    Count nrange = nullptr;
    {
        Lease lease(d, st);  // (handed on before the host waits)
        if (timed) HIP_OK(hipEventRecord(d.ev0, st));
        const int rc = run_spans(d, s, route, st, timed ? &nrange : nullptr, true, timed ? d.ev1 : nullptr);
        if (rc || !timed) return rc;
    }
    HIP_OK(hipEventSynchronize(d.ev1));
    if (nrange) HIP_OK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&g_last_kernel_ms, d.ev0, d.ev1);
    return nrange && *nrange ? CRC32C_ERANGE : CRC32C_OK;
}

}  // namespace
