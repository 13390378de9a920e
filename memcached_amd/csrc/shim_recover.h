// shim_recover.h -- recover_pages, the body of crc32c_recover_pages and, with
// `triage`, of crc32c_triage_pages (the pick is then shim_triage.h's and the
// merge takes its kind bytes, every other launch is the same): the page
// walk and its verify (shim_walk.h), the salvage's stages behind them
// (shim_salvage.h SalvageRun) and the merge of the two lists (k_recover.h),
// under one lock and one lease.  A host buffer is staged once, by the walk;
// the walk's offsets and verdicts stay in walk scratch and feed the salvage as
// device pointers; what comes back are the counts that size the next stage
// and, last, one copy of the merged results (the contract:
// include/crc32c_batch.h).
#pragma once

namespace {

static_assert(mcrc_dev::kKindSalvaged == CRC32C_ITEM_SALVAGED, "the merge writes the header's kind");

// What recover_stages leaves: the counts, the call's status, and the merged
// list's device arrays (`out`, with the entries written in out.cap).
struct PageLists {
    uint64_t total = 0, np = 0, nf = 0, nb = 0, sc = 0, nc = 0;  // walked, picked, found among them, bad, scanned, candidates
    int ret = CRC32C_OK;  // CRC32C_OK, CRC32C_EWALK or CRC32C_EWORK: the lists are the walk's then
    mcrc_dev::RecoverOut out{nullptr, nullptr, nullptr, 0};
};

// The call's stages under a lock and a lease already held: recover_pages below
// and crc32c_scrub_pages (shim_scrub.h) call it.  base: a device buffer with
// CRC32C_DEVICE in flags, else a host buffer, which the walk stages.  direct:
// the device arrays that take the merged list's first direct->cap entries, or
// nullptr: scratch takes its first cap (UINT64_MAX: the whole list).  Returns
// with the stream drained.
int recover_stages(Device &d, hipStream_t st, const void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t nw,
                   bool triage, unsigned flags, const mcrc_dev::RecoverOut *direct, uint64_t cap, PageLists *p) {
    int rc;
    // the walk and its verify: the lists stay in walk scratch
    mcrc_dev::SpanArgs a;
    mcrc_dev::WalkOut wo;
    uint32_t walked_n = 0;
    if ((rc = walk_count(d, st, base, base_bytes, wbuf_bytes, nw, flags, &a, &wo, &walked_n))) return rc;
    const uint64_t total = walked_n;
    uint64_t *woffs = d.walk_offs.reserve((size_t)total * 8);
    uint8_t *wok = d.walk_ok.reserve(total);
    if (total && (!woffs || !wok)) return CRC32C_ENOMEM;
    Count count = nullptr;
    if (total && (rc = walk_items<1>(d, st, a, wo, nw, total, woffs, wok, nullptr, &count))) return rc;

    // the salvage's stages over them (per-piece scratch of its own: the walk's scan is still in use)
    SalvageRun r{d, st};
    r.wpre = wo.prefix;
    if ((rc = r.init(item_args(d, a.base, base_bytes, wbuf_bytes, 0, flags), woffs, wok, total, nw, d.rc_cnt, d.rc_pre,
                     d.rc_slots)))
        return rc;
    if ((rc = r.regions(false))) return rc;
    // (the stream has drained: the walk's counts, before the candidates' verify writes the same words)
    const uint64_t nb = total ? count[0] : 0;
    int ret = total && count[1] ? CRC32C_EWALK : CRC32C_OK;
    uint64_t *found = nullptr;
    TriagePick tp;
    if (ret == CRC32C_OK && r.ntiles) {
        if ((rc = r.scan())) return rc;
        if (r.nc && r.over()) {
            ret = CRC32C_EWORK;
        } else if (r.nc && triage) {
            if ((rc = r.candidates()) || (rc = triage_pick(r, woffs, &tp))) return rc;
            found = tp.picked;
        } else if (r.nc) {
            if (!(found = d.sv_out.reserve(r.nc * 8))) return CRC32C_ENOMEM;
            if ((rc = r.candidates()) || (rc = r.pick(found, r.nc))) return rc;
            HIP_OK(hipMemcpyAsync(r.h32, r.ppre + nw, 4, hipMemcpyDeviceToHost, st));
        }
    }

    // the merge: into the caller's device arrays, or into scratch of the entries a host caller takes
    const uint64_t most = total + (found ? r.nc : 0), kcap = std::min(direct ? direct->cap : cap, most);
    mcrc_dev::RecoverOut out{nullptr, nullptr, nullptr, 0};
    if (direct) out = *direct;
    if (!direct && kcap) {
        out = mcrc_dev::RecoverOut{d.rc_offs.reserve(kcap * 8), d.rc_lens.reserve(kcap * 4), d.rc_kind.reserve(kcap),
                                   kcap};
        if (!out.offsets || !out.lens || !out.kind) return CRC32C_ENOMEM;
    }
    if (kcap) {
        // a workgroup per 1024 entries or more (four rounds of its threads: k_recover.h), 2048 workgroups at the most
        const uint64_t grid = std::min<uint64_t>((most + 1023) / 1024, 2048), per = (most + grid - 1) / grid;
        // (tp.kind: the picked entries' kinds, nullptr unless the triage picked: all of them are kind 4 then)
        hipLaunchKernelGGL(mcrc_dev::k_recover_merge, dim3((unsigned)grid), dim3(256), 0, st, a,
                           (const uint64_t *)woffs, (const uint8_t *)wok, wo.prefix, nw, (const uint64_t *)found,
                           (const uint8_t *)tp.kind, found ? (const uint32_t *)r.ppre : (const uint32_t *)nullptr,
                           (const uint64_t *)r.cand, (const uint32_t *)r.cand_nt, r.nc, per, out);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipStreamSynchronize(st));
    // (triage: h32[0] is the picked entries, found and suspects together, h32[1] the found among them)
    p->total = total;
    p->np = found ? r.h32[0] : 0;
    p->nf = triage && found ? r.h32[1] : p->np;
    p->nb = nb;
    p->sc = r.sc;
    p->nc = r.nc;
    p->ret = ret;
    p->out = out;
    return CRC32C_OK;
}

int recover_pages(const void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t *offsets, uint32_t *lens,
                  uint8_t *kind, uint64_t cap, uint64_t *nitems, uint64_t *nbad, uint64_t *nsalvaged,
                  uint64_t *nsuspect, bool triage, uint64_t *scanned, uint64_t *ncand, unsigned flags,
                  void *stream) {
    if (!base || !nitems || !nbad || !nsalvaged || !wbuf_bytes || (cap && (!offsets || !lens || !kind)) ||
        (triage && !nsuspect))
        return CRC32C_EINVAL;
    Device *dp = nullptr;
    int rc = current_device(&dp);
    if (rc) return rc;
    Device &d = *dp;
    hipStream_t st = (hipStream_t)stream;
    const bool dev = flags & CRC32C_DEVICE;
    if (dev && !device_range_ok(base, base_bytes)) return CRC32C_EINVAL;
    auto done = [&](uint64_t ni, uint64_t nb, uint64_t ns, uint64_t sc, uint64_t nc, int ret, uint64_t nsus = 0) {
        *nitems = ni;
        *nbad = nb;
        *nsalvaged = ns;
        if (triage) *nsuspect = nsus;
        if (scanned) *scanned = sc;
        if (ncand) *ncand = nc;
        return ret;
    };
    const uint64_t nw = (base_bytes + wbuf_bytes - 1) / wbuf_bytes;
    if (nw == 0) return done(0, 0, 0, 0, 0, CRC32C_OK);
    if (nw >= 0x7fffffffull) return CRC32C_EINVAL;
    std::lock_guard<std::mutex> lk(d.mu);
    Lease lease(d, st, !dev);  // (host: every exit drains st, the copies read and write the caller's memory)

    const mcrc_dev::RecoverOut mine{offsets, lens, kind, cap};
    PageLists p;
    if ((rc = recover_stages(d, st, base, base_bytes, wbuf_bytes, nw, triage, flags, dev ? &mine : nullptr, cap, &p)))
        return rc;
    const uint64_t k = std::min(cap, p.total + p.np);
    if (!dev && k) {
        HIP_OK(hipMemcpy(offsets, p.out.offsets, k * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(lens, p.out.lens, k * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(kind, p.out.kind, k, hipMemcpyDeviceToHost));
    }
    return done(p.total + p.np, p.nb, p.nf, p.sc, p.nc, p.ret, p.np - p.nf);
}

}  // namespace
