// shim_scrub.h -- scrub_pages, the body of crc32c_scrub_pages: the triage
// (recover_stages, shim_recover.h), the header repair (header_stages,
// shim_header.h) and the item repair (item_stages, shim_repair.h) in the loop
// of the contract (include/crc32c_batch.h), under one lock and one lease.  A
// host page is staged once, before the first triage; every stage then runs on
// device memory and writes in place.  The merged list stays in the recover
// call's scratch, whole; the two repair lists are built from it on the device
// (k_scrub.h), and each repair stage's verdicts are compacted into the log
// there too.  Between stages only the counts that size the next one cross the
// link: the triage's totals, a list's length, a stage's nrepaired (a host
// call also takes each round's flips, 17 B apiece, to invert them in the
// caller's buffer at the end).
// Scratch (grow-only) beyond the three calls': per entry of the merged list
// 13 B (rc_offs, rc_lens, rc_kind at the whole list's size); per piece 8 B of
// count and scan; per repair-list entry 8 B of offset, and the verdicts in
// the repair calls' own host-route scratch (hd_ok, hd_bit, hd_lens; rp_ok,
// rp_bit); a host call: the staged page and 17 B per flip of a round.
// CRC32C_SCRUB_GAPS (opts->mode): after each triage the gap starts are counted
// once (one count, 4 B, crosses the link); where there are any, they are
// emitted and merged with the triage's list into a second list, and both
// repair lists of that T are built from it, by the same two kernels.  With
// none, or with the bit clear, the launches are the ones above (with the bit
// set, one count launch, one scan and one 4 B copy more per triage).  Scratch
// (grow-only): 12 B per gap entry (offset and length; the kind is written by
// the merge), and 14 B per entry of the second list (offset, length and a kind
// array per repair stage).
// CRC32C_SCRUB_BYTES (opts->mode): when the item stage of a T repaired nothing,
// crc32c_repair_bytes' rule runs over the same list, still in sc_list (no
// second build): item_stages with the mask array, then k_scrub_log_bytes,
// which expands each repaired entry's mask into one log entry per bit and
// returns the stage's bit count (8 B cross the link; a host call takes that
// many flips).  With the bit clear no launch, copy or reservation is added.
// Scratch (grow-only): 1 B of mask per item-list entry, 8 B of count and its
// pinned twin, and a host call 8 flip slots per image the stage repaired.
#pragma once

namespace {

static_assert(CRC32C_SCRUB_BY_HEADER != CRC32C_SCRUB_BY_ITEM && CRC32C_SCRUB_BY_BYTE != CRC32C_SCRUB_BY_HEADER &&
                  CRC32C_SCRUB_BY_BYTE != CRC32C_SCRUB_BY_ITEM,
              "the log tells the stages apart");
static_assert(!(CRC32C_SCRUB_BYTES & (CRC32C_DEVICE | CRC32C_ASYNC | CRC32C_CFLAGS64 | CRC32C_KEEP_STAMPED |
                                      CRC32C_LOCATE_ONLY | CRC32C_SCRUB_GAPS)),
              "a mode bit of its own");
static_assert(CRC32C_REPAIR_BYTES_SPAN_DEFAULT <= CRC32C_REPAIR_SPAN_DEFAULT,
              "the byte stage's span limit is at most the item stage's: its work sum too");

struct ScrubRun {
    Device &d;
    hipStream_t st;
    uint8_t *page;  // device memory: the caller's, or the staged copy
    uint64_t base_bytes, wbuf_bytes, nw;
    unsigned flags;  // CRC32C_DEVICE and the caller's CRC32C_CFLAGS64
    bool dev;
    crc32c_scrub_out *o;  // the caller's arrays
    uint32_t *h32 = nullptr;
    uint64_t *list = nullptr;  // the repair list in use
    uint64_t items_n = 0;      // the item list's length, of the T whose item stage ran last
    bool gaps = false;         // CRC32C_SCRUB_GAPS
    bool gaps_known = false;   // of the T in hand: ng and, when ng != 0, the second list
    uint64_t ng = 0;
    mcrc_dev::ScrubList second{nullptr, nullptr, nullptr, 0};  // (kind: the headers')
    const uint8_t *second_ikind = nullptr;                       // the items' kind array of it
    uint64_t nflips = 0;
    std::vector<uint64_t> foff, fbit;  // a host call's log
    std::vector<uint8_t> fby;

    int triage(PageLists *t, float *ms) {
        const int rc = recover_stages(d, st, page, base_bytes, wbuf_bytes, nw, true, flags, nullptr, UINT64_MAX, t);
        *ms = g_last_kernel_ms;
        gaps_known = false;
        return rc;
    }

    // gap_starts(T), and T with them as the second list
    int gap_list(const mcrc_dev::ScrubList &l) {
        gaps_known = true;
        ng = 0;
        if (l.n == 0) return CRC32C_OK;  // (no kind-4 entry)
        uint32_t *cnt = d.sc_cnt.reserve(nw * 4), *pre = d.sc_pre.reserve((nw + 1) * 4);
        if (!cnt || !pre) return CRC32C_ENOMEM;
        const mcrc_dev::SpanArgs a = item_args(d, page, base_bytes, wbuf_bytes, 0, flags);
        const dim3 grid(mcrc::walk_grid(nw)), block(64 * mcrc_dev::kWalkWaves);
        hipLaunchKernelGGL(mcrc_dev::k_scrub_gaps<false>, grid, block, 0, st, a, l, nw, cnt, (const uint32_t *)nullptr,
                           mcrc_dev::RecoverOut{nullptr, nullptr, nullptr, 0});
        scan32(st, cnt, nw, pre);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(h32, pre + nw, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if ((ng = *h32) == 0) return CRC32C_OK;
        const uint64_t n2 = l.n + ng;
        const mcrc_dev::RecoverOut g{d.sc_goffs.reserve(ng * 8), d.sc_glens.reserve(ng * 4), nullptr, ng};
        const mcrc_dev::RecoverOut m{d.sc_moffs.reserve(n2 * 8), d.sc_mlens.reserve(n2 * 4), d.sc_mkind.reserve(n2),
                                     n2};
        uint8_t *ikind = d.sc_mikind.reserve(n2);
        if (!g.offsets || !g.lens || !m.offsets || !m.lens || !m.kind || !ikind) return CRC32C_ENOMEM;
        hipLaunchKernelGGL(mcrc_dev::k_scrub_gaps<true>, grid, block, 0, st, a, l, nw, (uint32_t *)nullptr,
                           (const uint32_t *)pre, g);
        const uint64_t mgrid = std::min<uint64_t>((n2 + 255) / 256, 2048);
        hipLaunchKernelGGL(mcrc_dev::k_scrub_gap_merge, dim3((unsigned)mgrid), dim3(256), 0, st, l,
                           (const uint64_t *)g.offsets, (const uint32_t *)g.lens, ng, m, ikind);
        HIP_OK(hipGetLastError());
        second = mcrc_dev::ScrubList{m.offsets, m.lens, m.kind, n2};
        second_ikind = ikind;
        return CRC32C_OK;
    }

    // header_list(T) or item_list(T) into `list`; *n: its length
    template <bool ITEMS>
    int build(const PageLists &t, uint64_t *n) {
        mcrc_dev::ScrubList l{t.out.offsets, t.out.lens, t.out.kind, t.total + t.np};
        if (gaps && !gaps_known) {
            const int rc = gap_list(l);
            if (rc) return rc;
        }
        const bool g = gaps && ng != 0;  // (the lists of the second list)
        if (g) l = second;
        if (g && ITEMS) l.kind = second_ikind;
        uint32_t *cnt = d.sc_cnt.reserve(nw * 4), *pre = d.sc_pre.reserve((nw + 1) * 4);
        if (!cnt || !pre) return CRC32C_ENOMEM;
        const dim3 grid(mcrc::walk_grid(nw)), block(64 * mcrc_dev::kWalkWaves);
        auto launch = [&](auto kern, uint32_t *c, const uint32_t *p, uint64_t *out, uint64_t cap) {
            hipLaunchKernelGGL(kern, grid, block, 0, st, l, wbuf_bytes, base_bytes, nw, c, p, out, cap);
        };
        using namespace mcrc_dev;
        launch(ITEMS ? k_scrub_items<false> : k_scrub_headers<false>, cnt, nullptr, nullptr, 0);
        scan32(st, cnt, nw, pre);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(h32, pre + nw, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        *n = *h32;
        if (*n == 0) return CRC32C_OK;
        if (!(list = d.sc_list.reserve(*n * 8))) return CRC32C_ENOMEM;
        launch(ITEMS ? k_scrub_items<true> : k_scrub_headers<true>, nullptr, pre, list, *n);
        HIP_OK(hipGetLastError());
        return CRC32C_OK;
    }

    // a stage's nrep flips behind the log's nflips: into the caller's device
    // arrays, or through a round's scratch into the host's log
    int log(const uint8_t *ok, const uint64_t *bit, uint64_t n, uint64_t nrep, uint32_t by) {
        uint64_t *fo = o->flip_offsets, *fb = o->flip_bits;
        uint8_t *fy = o->flip_by;
        uint64_t at = nflips, cap = o->flip_cap;
        if (!dev) {
            fo = d.sc_foff.reserve(nrep * 8);
            fb = d.sc_fbit.reserve(nrep * 8);
            fy = d.sc_fby.reserve(nrep);
            if (!fo || !fb || !fy) return CRC32C_ENOMEM;
            at = 0;
            cap = nrep;
        }
        if (at < cap) {
            hipLaunchKernelGGL(mcrc_dev::k_scrub_log, dim3(1), dim3(mcrc_dev::kScrubLogThreads), 0, st,
                               (const uint64_t *)list, ok, bit, n, by, at, cap, fo, fb, fy);
            HIP_OK(hipGetLastError());
        }
        if (!dev) {
            const int rc = take(fo, fb, fy, nrep);
            if (rc) return rc;
        }
        nflips += nrep;
        return CRC32C_OK;
    }

    // a host call's k flips of one stage, from its scratch to the host's log behind nflips
    int take(const uint64_t *fo, const uint64_t *fb, const uint8_t *fy, uint64_t k) {
        foff.resize(nflips + k);
        fbit.resize(nflips + k);
        fby.resize(nflips + k);
        HIP_OK(hipMemcpyAsync(foff.data() + nflips, fo, k * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(fbit.data() + nflips, fb, k * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(fby.data() + nflips, fy, k, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return CRC32C_OK;
    }

    // a byte stage's flips behind the log's nflips, one per set bit of each
    // of its nrep masks: at most 8 nrep, the exact count comes back from the kernel
    int log_bytes(const uint8_t *ok, const uint64_t *byte, const uint8_t *mask, uint64_t n, uint64_t nrep) {
        uint64_t *fo = o->flip_offsets, *fb = o->flip_bits;
        uint8_t *fy = o->flip_by;
        uint64_t at = nflips, cap = o->flip_cap;
        unsigned long long *nbits = d.sc_nbits.reserve(8), *h = d.sc_hbits.reserve(8);
        if (!nbits || !h) return CRC32C_ENOMEM;
        if (!dev) {
            fo = d.sc_foff.reserve(8 * nrep * 8);
            fb = d.sc_fbit.reserve(8 * nrep * 8);
            fy = d.sc_fby.reserve(8 * nrep);
            if (!fo || !fb || !fy) return CRC32C_ENOMEM;
            at = 0;
            cap = 8 * nrep;
        }
        hipLaunchKernelGGL(mcrc_dev::k_scrub_log_bytes, dim3(1), dim3(mcrc_dev::kScrubLogThreads), 0, st,
                           (const uint64_t *)list, ok, byte, mask, n, (uint32_t)CRC32C_SCRUB_BY_BYTE, at, cap, fo, fb,
                           fy, nbits);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(h, nbits, 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        const uint64_t k = *h;
        if (!dev) {
            const int rc = take(fo, fb, fy, k);
            if (rc) return rc;
        }
        nflips += k;
        return CRC32C_OK;
    }

    // one repair stage over T's list; *status: the repair call's own (CRC32C_EWORK, CRC32C_EINVAL), *nrep: what it repaired
    template <bool ITEMS>
    int repair(const PageLists &t, uint32_t max_span, int *status, uint64_t *nrep) {
        uint64_t n = 0;
        int rc = build<ITEMS>(t, &n);
        if (rc) return rc;
        *status = CRC32C_OK;
        *nrep = 0;
        if (ITEMS) items_n = n;
        if (n == 0) return CRC32C_OK;
        mcrc_dev::SpanArgs a = item_args(d, page, base_bytes, wbuf_bytes, n, flags);
        a.offsets = list;
        unsigned long long *h = nullptr;
        uint8_t *ok;
        uint64_t *bit;
        if (ITEMS) {
            const mcrc::ItemRoute route = mcrc::item_route(n, base_bytes, small_max(), false);
            ok = d.rp_ok.reserve(n);
            bit = d.rp_bit.reserve(n * 8);
            if (route == mcrc::ItemRoute::invalid) {
                *status = CRC32C_EINVAL;
                return CRC32C_OK;
            }
            if (!ok || !bit) return CRC32C_ENOMEM;
            bool searched = false;
            rc = item_stages(d, st, a, base_bytes, n, route, max_span, ok, bit, false, &h, &searched);
        } else {
            ok = d.hd_ok.reserve(n);
            bit = d.hd_bit.reserve(n * 8);
            uint32_t *lens = d.hd_lens.reserve(n * 4);
            if (n > mcrc::kHeaderListMax) {
                *status = CRC32C_EINVAL;
                return CRC32C_OK;
            }
            if (!ok || !bit || !lens) return CRC32C_ENOMEM;
            rc = header_stages(d, st, a, base_bytes, n, ok, bit, lens, false, &h);
        }
        if (rc == CRC32C_EWORK) {
            *status = rc;
            return CRC32C_OK;
        }
        if (rc) return rc;
        HIP_OK(hipStreamSynchronize(st));
        *nrep = h[ITEMS ? (int)mcrc_dev::kRpRepaired : (int)mcrc_dev::kHdRepaired];
        if (*nrep) rc = log(ok, bit, n, *nrep, ITEMS ? CRC32C_SCRUB_BY_ITEM : CRC32C_SCRUB_BY_HEADER);
        return rc;
    }

    // crc32c_repair_bytes' rule over the list the item stage of this T just
    // ran on (list, items_n: nothing was built since); bspan: the resolved limit
    int repair_bytes(uint32_t bspan, int *status, uint64_t *nrep) {
        const uint64_t n = items_n;
        *status = CRC32C_OK;
        *nrep = 0;
        if (n == 0) return CRC32C_OK;
        mcrc_dev::SpanArgs a = item_args(d, page, base_bytes, wbuf_bytes, n, flags);
        a.offsets = list;
        // (the item stage's route: it took this list)
        const mcrc::ItemRoute route = mcrc::item_route(n, base_bytes, small_max(), false);
        uint8_t *ok = d.rp_ok.reserve(n), *mask = d.rp_mask.reserve(n);
        uint64_t *byte = d.rp_bit.reserve(n * 8);
        if (!ok || !byte || !mask) return CRC32C_ENOMEM;
        unsigned long long *h = nullptr;
        bool searched = false;
        int rc = item_stages(d, st, a, base_bytes, n, route, bspan, ok, byte, false, &h, &searched, mask);
        if (rc == CRC32C_EWORK) {
            *status = rc;
            return CRC32C_OK;
        }
        if (rc) return rc;
        HIP_OK(hipStreamSynchronize(st));
        *nrep = h[mcrc_dev::kRpRepaired];
        if (*nrep) rc = log_bytes(ok, byte, mask, n, *nrep);
        return rc;
    }
};

int scrub_pages(void *base, uint64_t base_bytes, uint64_t wbuf_bytes, const crc32c_scrub_opts *opts,
                crc32c_scrub_out *out) {
    static const crc32c_scrub_opts none{};
    const crc32c_scrub_opts &op = opts ? *opts : none;
    if (!base || !out || !wbuf_bytes || (out->cap && (!out->offsets || !out->lens || !out->kind)) ||
        (out->flip_cap && (!out->flip_offsets || !out->flip_bits || !out->flip_by)) ||
        op.max_span > CRC32C_REPAIR_SPAN_MAX)
        return CRC32C_EINVAL;
    Device *dp = nullptr;
    int rc = current_device(&dp);
    if (rc) return rc;
    Device &d = *dp;
    const bool dev = op.mode & CRC32C_DEVICE, locate_only = op.mode & CRC32C_LOCATE_ONLY;
    if (dev && (locate_only || !device_range_ok(base, base_bytes))) return CRC32C_EINVAL;
    const uint64_t nw = (base_bytes + wbuf_bytes - 1) / wbuf_bytes;
    if (nw >= 0x7fffffffull) return CRC32C_EINVAL;
    const uint32_t max_rounds = op.max_rounds ? op.max_rounds : CRC32C_SCRUB_ROUNDS_DEFAULT;
    const bool bytes = op.mode & CRC32C_SCRUB_BYTES;
    const uint32_t bspan = op.max_span ? std::min<uint32_t>(op.max_span, CRC32C_REPAIR_BYTES_SPAN_DEFAULT)
                                       : CRC32C_REPAIR_BYTES_SPAN_DEFAULT;

    PageLists t;
    uint64_t headers_repaired = 0, items_repaired = 0, nflips = 0;
    uint32_t rounds = 0, complete = 0;
    auto done = [&](int ret) {
        out->nitems = t.total + t.np;
        out->nbad = t.nb;
        out->nsalvaged = t.nf;
        out->nsuspect = t.np - t.nf;
        out->scanned = t.sc;
        out->ncand = t.nc;
        out->nflips = nflips;
        out->headers_repaired = headers_repaired;
        out->items_repaired = items_repaired;
        out->rounds = rounds;
        out->complete = complete;
        return ret;
    };
    if (nw == 0) {
        complete = 1;
        return done(CRC32C_OK);
    }
    std::lock_guard<std::mutex> lk(d.mu);
    hipStream_t st = dev ? (hipStream_t)op.stream : d.stream;  // (device: NULL is the default stream)
    if (!dev) HIP_OK(hipSetDevice(d.id));
    Lease lease(d, st, !dev);  // (host: every exit drains st, the copies read and write the caller's memory)

    ScrubRun r{d, st, (uint8_t *)base, base_bytes, wbuf_bytes, nw,
               (unsigned)CRC32C_DEVICE | (op.mode & (unsigned)CRC32C_CFLAGS64), dev, out};
    r.gaps = op.mode & CRC32C_SCRUB_GAPS;
    if (!(r.h32 = d.sc_host.reserve(4))) return CRC32C_ENOMEM;
    if (!dev) {  // the one staging of the page
        if (!(r.page = d.stage.reserve(base_bytes))) return CRC32C_ENOMEM;
        HIP_OK(hipMemcpyAsync(r.page, base, base_bytes, hipMemcpyHostToDevice, st));
    }

    float ms = 0.0f;  // (crc32c_last_kernel_ms: the last triage's counting pass)
    int status = CRC32C_OK;
    if ((rc = r.triage(&t, &ms))) return rc;
    for (;;) {
        if ((status = t.ret) != CRC32C_OK) break;
        uint64_t nrep = 0;
        if ((rc = r.repair<false>(t, 0, &status, &nrep))) return rc;
        if (status != CRC32C_OK) break;
        if (nrep == 0) {  // (headers before items, every time)
            if ((rc = r.repair<true>(t, op.max_span, &status, &nrep))) return rc;
            if (status != CRC32C_OK) break;
            if (nrep == 0 && bytes) {  // (the same list, the byte rule)
                if ((rc = r.repair_bytes(bspan, &status, &nrep))) return rc;
                if (status != CRC32C_OK) break;
            }
            if (nrep == 0) {
                complete = 1;  // (T describes the page: no further triage)
                break;
            }
            items_repaired += nrep;
        } else {
            headers_repaired += nrep;
        }
        ++rounds;
        if ((rc = r.triage(&t, &ms))) return rc;
        if (rounds == max_rounds) break;
    }
    if (status == CRC32C_OK) status = t.ret;
    nflips = r.nflips;

    // the final list's first cap entries, and a host call's log and inversions
    const uint64_t k = std::min(out->cap, t.total + t.np), kf = std::min(out->flip_cap, nflips);
    if (k) {
        const hipMemcpyKind to = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        HIP_OK(hipMemcpyAsync(out->offsets, t.out.offsets, k * 8, to, st));
        HIP_OK(hipMemcpyAsync(out->lens, t.out.lens, k * 4, to, st));
        HIP_OK(hipMemcpyAsync(out->kind, t.out.kind, k, to, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    if (!dev) {
        if (!locate_only)
            for (uint64_t i = 0; i < nflips; ++i)
                ((uint8_t *)base)[r.foff[i] + r.fbit[i] / 8] ^= (uint8_t)(1u << (r.fbit[i] % 8));
        if (kf) {
            memcpy(out->flip_offsets, r.foff.data(), kf * 8);
            memcpy(out->flip_bits, r.fbit.data(), kf * 8);
            memcpy(out->flip_by, r.fby.data(), kf);
        }
    }
    g_last_kernel_ms = ms;
    return done(status);
}

}  // namespace
