// crc32c_shim.hip -- the C-ABI library (libmcrc32c.so): memcached's crc32c.h
// surface plus the batched gfx950 entry points of crc32c_batch.h.
//
// Host side of the drop-in boundary.  The scalar symbols replace crc32c.c
// (crc32c.c:47, :266-275, :507-513); the batch symbols replace loops of those
// calls in storage.c / proxy_internal.c (see include/crc32c_batch.h).
// This file is the index of the one translation unit (the includes and the
// extern "C" surface); host_route.h and the shim_*.h parts hold the rest.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/crc32c.h"
#include "../../include/crc32c_batch.h"
#include "crc32c_gf2.h"
#include "crc32c_host.h"
#include "grow_buf.h"
#include "host_route.h"
#include "k1_slots.h"
#include "crc32c_kernels.hip"

// Scalar drop-in (crc32c.h)
extern "C" {

crc_func crc32c = nullptr;

void crc32c_init(void) {
    mcrc::host_tables_init();
    crc32c = mcrc::host_has_hw_crc() ? mcrc::crc32c_host_hw : mcrc::crc32c_host_sw;
}

uint32_t crc32c_sw(uint32_t crc, void const *buf, size_t len) { return mcrc::crc32c_host_sw(crc, buf, len); }
uint32_t crc32c_sw_little(uint32_t crc, void const *buf, size_t len) { return mcrc::crc32c_host_sw(crc, buf, len); }
uint32_t crc32c_sw_big(uint32_t crc, void const *buf, size_t len) { return mcrc::crc32c_host_sw_big(crc, buf, len); }

}  // extern "C"

#include "shim_device.h"
#include "shim_launch.h"
#include "shim_host.h"
#include "shim_queue.h"
#include "shim_ptrs.h"
#include "shim_walk.h"
#include "shim_salvage.h"
#include "shim_triage.h"
#include "shim_recover.h"
#include "shim_repair.h"
#include "shim_header.h"
#include "shim_scrub.h"

// Batch C ABI
extern "C" {

int crc32c_gpu_count(void) {
    const int n = g_ngfx_pub.load(std::memory_order_acquire);
    if (n >= 0) return n;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    return ensure_devices();
}

void *crc32c_host_alloc(size_t bytes) {
    if (bytes == 0 || crc32c_gpu_count() <= 0) return nullptr;
    void *p = nullptr;
    // portable: usable by every device's copy engine (crc32c_batch_multi)
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) return nullptr;
    pin_record(p, bytes);
    return p;
}

void crc32c_host_free(void *p) {
    if (!p) return;
    pin_forget(p);
    (void)hipHostFree(p);
}

int crc32c_host_register(void *p, size_t bytes) {
    if (!p || !bytes) return CRC32C_EINVAL;
    if (crc32c_gpu_count() <= 0) return CRC32C_ENODEV;
    HIP_OK(hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    pin_record(p, bytes);
    return CRC32C_OK;
}

int crc32c_host_unregister(void *p) {
    if (!p) return CRC32C_EINVAL;
    if (crc32c_gpu_count() <= 0) return CRC32C_ENODEV;
    pin_forget(p);
    HIP_OK(hipHostUnregister(p));
    return CRC32C_OK;
}

uint64_t crc32c_set_small_max(uint64_t n) {
    return g_small_max.exchange(std::min<uint64_t>(n, mcrc_dev::kSmallMax));
}

uint64_t crc32c_set_k1_tail_min(uint64_t steps) {
    return g_k1_tail_min.exchange(std::max<uint64_t>(steps, mcrc_dev::kK1TailFloorSteps));
}

const char *crc32c_strerror(int err) {
    switch (err) {
        case CRC32C_OK: return "ok";
        case CRC32C_ENODEV: return "no gfx950 device";
        case CRC32C_EHIP: return "HIP runtime error";
        case CRC32C_EINVAL: return "invalid argument";
        case CRC32C_ENOMEM: return "out of device or pinned memory";
        case CRC32C_ERANGE: return "span outside [base, base + base_bytes) (not read)";
        case CRC32C_EWALK: return "device page walk passes disagreed (results not valid)";
        case CRC32C_EWORK: return "the candidates' or damaged images' spans exceed the work bound (nothing verified)";
        default: return "unknown error";
    }
}

float crc32c_last_kernel_ms(void) { return g_last_kernel_ms; }

int crc32c_batch_submit(const crc32c_spans *s, unsigned flags, crc32c_job_t *job) {
    if (!s || !job) return CRC32C_EINVAL;
    crc32c_job *j = nullptr;
    const int rc = make_job(*s, flags, &j);
    if (rc) return rc;
    if (!j->q->submit(j)) {
        if (j->after) (void)hipEventDestroy(j->after);
        delete j;
        return CRC32C_EHIP;
    }
    *job = j;
    return CRC32C_OK;
}

int crc32c_batch_wait(crc32c_job_t j) {
    if (!j) return CRC32C_EINVAL;
    const int rc = j->q->wait(j);
    delete j;
    return rc;
}

int crc32c_queue_stats(uint64_t *launches, uint64_t *spans, uint64_t *jobs, uint64_t *solo_jobs) {
    Device *d = nullptr;
    const int rc = current_device(&d);
    if (rc) return rc;
    const Queue *q = d->queue.load(std::memory_order_acquire);
    if (launches) *launches = q ? q->launches.load() : 0;
    if (spans) *spans = q ? q->spans.load() : 0;
    if (jobs) *jobs = q ? q->jobs.load() : 0;
    if (solo_jobs) *solo_jobs = q ? q->solo.load() : 0;
    return CRC32C_OK;
}

int crc32c_batch(const crc32c_spans *s, unsigned flags, void *stream) {
    if (!s || (s->n && (!s->base || !s->out))) return CRC32C_EINVAL;
    Device *d = nullptr;
    int rc = current_device(&d);
    if (rc) return rc;
    if (!(flags & CRC32C_DEVICE)) {
        // short spans in page-locked memory share the queue's launches with
        // other threads' batches; anything else is staged on its own
        crc32c_job *j = nullptr;
        if ((rc = make_job(*s, flags, &j))) return rc;
        if (!j->coalesce) {
            delete j;
            return run_host_batch(*d, *s);
        }
        rc = j->q->submit(j) ? j->q->wait(j) : CRC32C_EHIP;
        delete j;
        return rc;
    }
    // Device batches run on the caller's stream; NULL is the default stream, so
    // the kernel is ordered after whatever produced the buffers there.
    return device_batch(*d, *s, flags, (hipStream_t)stream);
}

int crc32c_batch_chains(const crc32c_spans *iovs, const uint64_t *chain_first, uint64_t nchains, uint32_t *out,
                        unsigned flags, void *stream) {
    if (!iovs || !chain_first || (nchains && !out) || iovs->crc_in) return CRC32C_EINVAL;
    if (nchains == 0) return CRC32C_OK;
    Device *d = nullptr;
    int rc = current_device(&d);
    if (rc) return rc;
    const bool dev = flags & CRC32C_DEVICE;
    if (!dev) {  // per-iov CRCs through the staged host path, then the fold on the device
        for (uint64_t c = 0; c < nchains; ++c)
            if (chain_first[c + 1] < chain_first[c] || chain_first[c + 1] > iovs->n) return CRC32C_EINVAL;
        rc = run_host_batch(*d, *iovs);
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> lk(d->mu);
    hipStream_t st = dev ? (hipStream_t)stream : d->stream;
    Lease lease(*d, st);
    Count nrange = nullptr;
    if (dev) {
        if (!device_range_ok(iovs->base, iovs->base_bytes)) return CRC32C_EINVAL;
        rc = run_spans(*d, *iovs, mcrc::span_route(*iovs, small_max()), st, (flags & CRC32C_ASYNC) ? nullptr : &nrange);
        if (rc) return rc;
    }
    return fold_chains(*d, iovs->out, iovs->lens, iovs->len, iovs->n, chain_first, nchains, out, dev, flags, st, nrange);
}

int crc32c_batch_ptrs(const crc32c_ptr_batch *b, const crc32c_ptr_opts *opts) {
    if (!b) return CRC32C_EINVAL;
    return batch_ptrs(*b, opts ? opts->mode : 0u, opts ? (hipStream_t)opts->stream : nullptr);
}

int crc32c_ptrs_submit(const crc32c_ptr_batch *b, const crc32c_ptr_opts *opts, crc32c_job_t *job) {
    if (!b || !job) return CRC32C_EINVAL;
    crc32c_job *j = nullptr;
    int rc = make_ptr_job(*b, opts ? opts->mode : 0u, &j);
    if (rc || (rc = submit_or_free(j))) return rc;
    *job = j;
    return CRC32C_OK;
}

int crc32c_chains_ptrs(const crc32c_ptr_batch *iovs, const uint64_t *chain_first, uint64_t nchains, uint32_t *out,
                       const crc32c_ptr_opts *opts) {
    if (!iovs || !chain_first || (nchains && !out) || iovs->crc_in) return CRC32C_EINVAL;
    if (nchains == 0) return CRC32C_OK;
    return chains_ptrs(*iovs, chain_first, nchains, out, opts ? opts->mode : 0u,
                       opts ? (hipStream_t)opts->stream : nullptr);
}

// (Stamp calls before verify calls: the kernel templates are laid out in the
// code object in the order their MODEs are first named, which tools/codeobj_diff.py compares too.)
int crc32c_stamp_items(void *base, uint64_t base_bytes, uint64_t region_bytes, const uint64_t *item_offsets,
                       uint64_t n, uint8_t *ok, uint64_t *nbad, unsigned flags, void *stream) {
    return with_stamp_mode(flags, [&](auto mode) {
        return item_images<mode()>(base, base_bytes, region_bytes, item_offsets, n, ok, nbad, flags, stream);
    });
}

int crc32c_verify_items(const void *base, uint64_t base_bytes, uint64_t region_bytes, const uint64_t *item_offsets,
                        uint64_t n, uint8_t *ok, uint64_t *nbad, unsigned flags, void *stream) {
    if (!nbad) return CRC32C_EINVAL;
    return item_images<1>(const_cast<void *>(base), base_bytes, region_bytes, item_offsets, n, ok, nbad,
                          flags & ~(unsigned)CRC32C_ASYNC, stream);
}

//   device: k_copy in place on the caller's stream;
//   host, both buffers page-locked and mapped (crc32c_host_alloc / _register:
//     extstore's readback_buf and wbufs): the same kernel through their mapped
//     addresses on the library stream;
//   host, otherwise: the verdicts come from the host verify route and the host
//     copies the sane images that fit with memcpy -- bytes already in host
//     memory cross the link once, for the check, and not again for the copy.
int crc32c_copy_items(const void *src, uint64_t src_bytes, uint64_t region_bytes, const uint64_t *src_offsets,
                      void *dst, uint64_t dst_bytes, const uint64_t *dst_offsets, uint64_t n, uint8_t *ok,
                      uint64_t *nbad, unsigned flags, void *stream) {
    if (!src || !dst || !src_offsets || !dst_offsets || !ok) return CRC32C_EINVAL;
    if (mcrc::ranges_overlap(src, src_bytes, dst, dst_bytes)) return CRC32C_EINVAL;
    Device *d = nullptr;
    int rc = current_device(&d);
    if (rc) return rc;
    if (n == 0) {
        if (nbad) *nbad = 0;
        return CRC32C_OK;
    }
    const bool dev = flags & CRC32C_DEVICE;
    if (dev && (!device_range_ok(src, src_bytes) || !device_range_ok(dst, dst_bytes))) return CRC32C_EINVAL;
    mcrc_dev::SpanArgs a = item_args(*d, src, src_bytes, region_bytes, n, flags);
    // the addresses k_copy uses: the device buffers, or both host buffers' mapped views
    const uint8_t *const msrc = dev ? a.base : device_view_range(src, src_bytes);
    const uint8_t *const mdst = dev ? (const uint8_t *)dst : msrc ? device_view_range(dst, dst_bytes) : nullptr;
    if (msrc && mdst) {
        std::lock_guard<std::mutex> lk(d->mu);
        hipStream_t st = dev ? (hipStream_t)stream : d->stream;  // (device: NULL is the default stream)
        if (!dev) HIP_OK(hipSetDevice(d->id));
        Count count = nullptr;
        {  // (the scratch is handed on before the host waits)
            Lease lease(*d, st, !dev);  // (host: every exit drains st first, the kernel writes pinned scratch)
            mcrc_dev::CopyArgs ca{};
            ca.dst = const_cast<uint8_t *>(mdst);
            ca.dst_bytes = dst_bytes;
            ca.dst_offsets = dst_offsets;
            a.base = msrc;
            a.offsets = src_offsets;
            a.ok = ok;
            if (!dev) {  // offsets and ok through pinned mapped scratch
                uint64_t *const h_offs = d->pin_offs.reserve(2 * n * 8);
                if (!h_offs || !d->pin_ok.reserve(n)) return CRC32C_ENOMEM;
                memcpy(h_offs, src_offsets, n * 8);
                memcpy(h_offs + n, dst_offsets, n * 8);
                a.offsets = d->pin_offs.dev();
                a.ok = d->pin_ok.dev();
                ca.dst_offsets = d->pin_offs.dev() + n;
            }
            if ((rc = run_copy(*d, a, ca, st, &count))) return rc;
            if (!dev) HIP_OK(hipStreamSynchronize(st));  // (before the lease's event: nothing waits for that)
        }
        if (dev && (flags & CRC32C_ASYNC) && !nbad) return CRC32C_OK;  // fire and forget
        if (dev) HIP_OK(hipStreamSynchronize(st));
        if (!dev) memcpy(ok, d->pin_ok.get(), n);
        if (nbad) *nbad = count[0];
        return count[1] ? CRC32C_ERANGE : CRC32C_OK;
    }
    uint64_t nv = 0;
    if ((rc = item_images<1>(const_cast<void *>(src), src_bytes, region_bytes, src_offsets, n, ok, &nv,
                             flags & ~(unsigned)CRC32C_ASYNC, nullptr)))
        return rc;
    uint64_t bad = 0;
    bool range = false;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t nt = 0;
        const bool sane = mcrc::item_sane((const uint8_t *)src, src_bytes, region_bytes, src_offsets[i], a.cfl, &nt);
        const bool fits = dst_offsets[i] <= dst_bytes && nt <= dst_bytes - dst_offsets[i];
        if (sane && fits) {
            memcpy((uint8_t *)dst + dst_offsets[i], (const uint8_t *)src + src_offsets[i], nt);
            ok[i] = ok[i] ? CRC32C_ITEM_COPIED : CRC32C_ITEM_DAMAGED;
        } else {
            ok[i] = 0;
            range |= sane;
        }
        bad += ok[i] != CRC32C_ITEM_COPIED;
    }
    if (nbad) *nbad = bad;
    return range ? CRC32C_ERANGE : CRC32C_OK;
}

int crc32c_stamp_pages(void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t *offsets, uint8_t *ok,
                       uint64_t cap, uint64_t *nitems, uint64_t *nbad, unsigned flags, void *stream) {
    return with_stamp_mode(flags, [&](auto mode) {
        return walk_pages<mode()>(base, base_bytes, wbuf_bytes, offsets, ok, cap, nitems, nbad, flags, stream);
    });
}

int crc32c_verify_pages(const void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t *offsets, uint8_t *ok,
                        uint64_t cap, uint64_t *nitems, uint64_t *nbad, unsigned flags, void *stream) {
    return walk_pages<1>(const_cast<void *>(base), base_bytes, wbuf_bytes, offsets, ok, cap, nitems, nbad, flags,
                         stream);
}

int crc32c_salvage_pages(const void *base, uint64_t base_bytes, uint64_t wbuf_bytes, const uint64_t *walked,
                         const uint8_t *walked_ok, uint64_t nwalked, uint64_t *offsets, uint64_t cap,
                         uint64_t *nfound, uint64_t *scanned, uint64_t *ncand, unsigned flags, void *stream) {
    return salvage_pages(base, base_bytes, wbuf_bytes, walked, walked_ok, nwalked, offsets, cap, nfound, scanned,
                         ncand, flags, stream);
}

int crc32c_recover_pages(const void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t *offsets, uint32_t *lens,
                         uint8_t *kind, uint64_t cap, uint64_t *nitems, uint64_t *nbad, uint64_t *nsalvaged,
                         uint64_t *scanned, uint64_t *ncand, unsigned flags, void *stream) {
    return recover_pages(base, base_bytes, wbuf_bytes, offsets, lens, kind, cap, nitems, nbad, nsalvaged, nullptr,
                         false, scanned, ncand, flags, stream);
}

int crc32c_triage_pages(const void *base, uint64_t base_bytes, uint64_t wbuf_bytes, uint64_t *offsets, uint32_t *lens,
                        uint8_t *kind, uint64_t cap, uint64_t *nitems, uint64_t *nbad, uint64_t *nsalvaged,
                        uint64_t *nsuspect, uint64_t *scanned, uint64_t *ncand, unsigned flags, void *stream) {
    return recover_pages(base, base_bytes, wbuf_bytes, offsets, lens, kind, cap, nitems, nbad, nsalvaged, nsuspect,
                         true, scanned, ncand, flags, stream);
}

int crc32c_repair_items(void *base, uint64_t base_bytes, uint64_t region_bytes, const uint64_t *item_offsets,
                        uint64_t n, uint32_t max_span, uint8_t *ok, uint64_t *bit, uint64_t *nrepaired, uint64_t *nbad,
                        unsigned flags, void *stream) {
    return repair_items(base, base_bytes, region_bytes, item_offsets, n, max_span, ok, bit, nrepaired, nbad, flags,
                        stream);
}

int crc32c_repair_bytes(void *base, uint64_t base_bytes, uint64_t region_bytes, const uint64_t *item_offsets,
                        uint64_t n, const crc32c_bytes_opts *opts, crc32c_bytes_out *out) {
    return repair_bytes(base, base_bytes, region_bytes, item_offsets, n, opts, out);
}

int crc32c_repair_headers(void *base, uint64_t base_bytes, uint64_t region_bytes, const uint64_t *item_offsets,
                          uint64_t n, uint8_t *ok, uint64_t *bit, uint32_t *lens, uint64_t *nrepaired, uint64_t *nbad,
                          unsigned flags, void *stream) {
    return repair_headers(base, base_bytes, region_bytes, item_offsets, n, ok, bit, lens, nrepaired, nbad, flags,
                          stream);
}

int crc32c_scrub_pages(void *base, uint64_t base_bytes, uint64_t wbuf_bytes, const crc32c_scrub_opts *opts,
                       crc32c_scrub_out *out) {
    return scrub_pages(base, base_bytes, wbuf_bytes, opts, out);
}

int crc32c_shard_cuts(const uint32_t *lens, uint32_t len, uint64_t n, int parts, uint64_t *cuts) {
    if (parts < 1 || !cuts) return CRC32C_EINVAL;
    mcrc::shard_cuts(lens, len, n, parts, cuts);
    return CRC32C_OK;
}

int crc32c_batch_multi(const crc32c_spans *s, int ngpus) {
    if (!s) return CRC32C_EINVAL;
    const int avail = crc32c_gpu_count();
    if (avail <= 0) return CRC32C_ENODEV;
    if (ngpus <= 0 || ngpus > avail) ngpus = avail;
    std::vector<uint64_t> cut(ngpus + 1);
    int rc = crc32c_shard_cuts(s->lens, s->len, s->n, ngpus, cut.data());
    if (rc) return rc;
    std::vector<int> rcs(ngpus, CRC32C_OK);
    MultiDone done;
    for (int g = 0; g < ngpus; ++g) {
        const uint64_t a0 = cut[g], a1 = cut[g + 1];
        if (a1 == a0) continue;
        crc32c_spans sub = *s;
        sub.n = a1 - a0;
        if (s->offsets) sub.offsets = s->offsets + a0;
        else {
            sub.base = (const uint8_t *)s->base + a0 * s->stride;
            sub.base_bytes = s->base_bytes - a0 * s->stride;
        }
        if (s->lens) sub.lens = s->lens + a0;
        if (s->crc_in) sub.crc_in = s->crc_in + a0;
        sub.out = s->out + a0;
        MultiWorker *w = multi_worker(g);
        if (!w) {
            rcs[g] = CRC32C_ENODEV;
            continue;
        }
        done.add();
        w->post(MultiJob{sub, &rcs[g], &done});
    }
    done.wait();
    for (int r : rcs)
        if (r) return r;
    return CRC32C_OK;
}

}  // extern "C"
