// shim_device.h -- per-device state and its lookup: the scratch buffers'
// memory policies, Device, Lease, init_device / current_device, HIP_OK and the
// pointer queries (is a range device memory, page-locked, mapped).
#pragma once

namespace {

// The memory sources of the shim's grow-only buffers (grow_buf.h).  Device
// blocks are freed with the synchronous hipFree: a regrow outlasts kernels
// still using the old block on another stream.
bool alloc_ok(hipError_t e) {
    if (e != hipSuccess) (void)hipGetLastError();  // (not left pending for a later launch check)
    return e == hipSuccess;
}
struct DeviceMem {
    static bool alloc(size_t bytes, mcrc::Block *b) {
        const bool ok = alloc_ok(hipMalloc(&b->p, bytes));
        b->dv = b->p;
        return ok;
    }
    static void free(const mcrc::Block &b) { (void)hipFree(b.p); }
};
struct PinnedMem {  // page-locked, for the host and the copy engines only
    static bool alloc(size_t bytes, mcrc::Block *b) {
        return alloc_ok(hipHostMalloc(&b->p, bytes, hipHostMallocDefault));
    }
    static void free(const mcrc::Block &b) { (void)hipHostFree(b.p); }
};
struct MappedMem : PinnedMem {  // page-locked and mapped: dev() is the address kernels use
    static bool alloc(size_t bytes, mcrc::Block *b) {
        if (!PinnedMem::alloc(bytes, b)) return false;
        if (alloc_ok(hipHostGetDevicePointer(&b->dv, b->p, 0))) return true;
        free(*b);
        return false;
    }
};
template <class T = uint8_t> using DevBuf = mcrc::GrowBuf<DeviceMem, T>;
template <class T = uint8_t> using PinBuf = mcrc::GrowBuf<PinnedMem, T>;
template <class T = uint8_t> using MapBuf = mcrc::GrowBuf<MappedMem, T>;

struct Queue;

struct Device {
    int id = -1;
    int cus = 0;
    bool ok = false;
    uint4 *img = nullptr;       // LDS table image of every table kernel (build_lds_image_span, chunk 16)
    uint32_t *tab8 = nullptr;   // byte-wise table (k_count / k_final: a span's head fragment and foreign bytes)
    uint32_t *xpow = nullptr;   // x^(8n) table (layout mcrc_dev::kXpow*)
    uint32_t *segpow = nullptr; // rows x^i * x^(8*4096*k): k < 256, then k = 256 j
    uint32_t xm128 = 0;         // k_lines / k_fix: x^(-8 * 128)
    uint4 *zero = nullptr;      // kZeroBytes of zeros (one 4 KiB line set per CU slot)
    unsigned long long *nbad = nullptr;  // [0]: bad / out-of-range count, [1]: walk invariant failures
    unsigned long long *hbad = nullptr;  // pinned twin of nbad[0..1] (a D2H copy into pageable memory is a slow path)
    // k_small's own counters for calls that take the count from hbad (item
    // images): zero between calls, kept so by the kernel's last workgroup
    unsigned long long *small_nbad = nullptr;
    uint32_t *small_done = nullptr;  // ([1]: k_copy's count of images that did not fit dst, kept the same way)
    // K1's claimed tail: a counter block per stream (k1_slots.h), zero between
    // launches, kept so by the kernel's last workgroup; the table is the one
    // piece of state a launch (const Device &, no mu) writes
    mcrc_dev::K1Ctl *k1_ctl = nullptr;
    mutable mcrc::K1Slots k1_slots;
    uint32_t *nfb = nullptr;    // k_lines' fallback count (device)
    uint32_t *route = nullptr;  // k_census's verdict: K5 (1) or the planned path (0)
    hipStream_t stream = nullptr, copy = nullptr;
    // a stamp's k_fix runs on `side` beside the damaged images' planned path
    // (fork: after k_lines on the caller's stream; join: the caller's stream
    // waits for it before the call's last kernel)
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t copied[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};  // host-batch pipeline slots
    std::mutex mu;              // serialises the entry points that use the scratch below
    std::atomic<Queue *> queue{nullptr};  // coalescing queue (crc32c_batch_submit), created on first use
    // Shared device scratch (plan buffers, nbad, walk buffers) is owned in
    // stream order: a launch on stream B waits for the last use on stream A.
    hipEvent_t busy = nullptr;
    hipStream_t busy_stream = nullptr;
    bool busy_valid = false;
    void acquire(hipStream_t st) {
        if (busy_valid && busy_stream != st) (void)hipStreamWaitEvent(st, busy, 0);
    }
    void release(hipStream_t st) {
        if (hipEventRecord(busy, st) == hipSuccess) {
            busy_stream = st;
            busy_valid = true;
        }
    }
    // Everything below is grow-only scratch (grow_buf.h), sized by the call
    // that needs it and guarded by mu and the stream-order hand-over above.
    // host-batch staging: two device slots + two pinned slots
    DevBuf<> dbuf[2];
    PinBuf<> pin[2];
    DevBuf<uint64_t> doffs[2];
    DevBuf<uint32_t> dlens[2], dcin[2], dout[2];
    PinBuf<uint64_t> hoffs[2];  // pinned twins of the descriptor slots
    PinBuf<uint32_t> hlens[2], hcin[2], hout[2];
    // work-unit planning for long / variable spans
    DevBuf<uint64_t> nunit;  // per span: units | blocks << 32
    DevBuf<mcrc_dev::PlanSum> tile_sum, tile_pre;  // per kPlanTile spans: sums, exclusive scan (+ total)
    DevBuf<uint32_t> span_acc, counters;
    DevBuf<uint32_t> starts;  // balanced plan: first record of each span-kernel group (groups + 1)
    DevBuf<mcrc_dev::UnitRec> units, whole;
    DevBuf<uint4> irec;  // per-span record written by k_count
    DevBuf<uint8_t> fast;      // per span: its unit is one whole block (k_blocks takes it)
    DevBuf<uint32_t> fastidx;  // the fast spans' indices, compacted (k_expand)
    DevBuf<uint4> big;  // spans expanded by k_expand_big: {span, p0, b0}
    // the page walk (counts, their scan, the slots the count pass keeps, and
    // the results when the caller's arrays do not take them)
    DevBuf<uint32_t> walk_cnt, walk_prefix;
    DevBuf<uint64_t> walk_slots, walk_offs;
    DevBuf<uint8_t> walk_ok;
    // staged host buffers (item images, pages, a chain fold's inputs) and the
    // staged item batches' offsets and results
    DevBuf<> stage, item_out;
    DevBuf<uint64_t> item_offs;
    // launch_items: the images K5 leaves to the planned path (indices, offsets,
    // verdicts) and a stamp's per-image records for k_fix
    DevBuf<uint32_t> fb;
    DevBuf<uint64_t> fb_offs;
    DevBuf<uint8_t> fb_ok;
    DevBuf<uint2> rt;
    // crc32c_salvage_pages: staged host lists, the counters and their pinned
    // twin, the tiles with their candidate counts and scan, the candidates
    // (offset, ntotal, verdict) and a host call's offsets found
    DevBuf<uint64_t> sv_walked, sv_cand, sv_out;
    DevBuf<uint8_t> sv_wok, sv_ok;
    DevBuf<unsigned long long> sv_ctr;
    PinBuf<unsigned long long> sv_host;
    DevBuf<mcrc_dev::SalvageTile> sv_tiles;
    DevBuf<uint32_t> sv_tcnt, sv_tpre, sv_nt;
    // crc32c_recover_pages: the salvage's per-piece counts, scan and kept ranges
    // (the walk's own hold its lists' layout until the merge) and a host
    // call's merged results
    DevBuf<uint32_t> rc_cnt, rc_pre, rc_lens;
    DevBuf<uint64_t> rc_slots, rc_offs;
    DevBuf<uint8_t> rc_kind;
    // crc32c_triage_pages: the kind byte beside each picked candidate and the
    // scan of the per-piece counts of the found among them
    DevBuf<uint8_t> tr_kind;
    DevBuf<uint32_t> tr_fpre;
    // crc32c_repair_items: per image its CRC, the two counts and their scans; per
    // listed image its record, first chunk and located t; the counters and
    // their pinned twin; a host call's verdicts and positions
    DevBuf<uint32_t> rp_crc, rp_lcnt, rp_ccnt, rp_lpre, rp_cpre, rp_first, rp_found;
    DevBuf<mcrc_dev::RepairRec> rp_recs;
    DevBuf<unsigned long long> rp_ctr;
    PinBuf<unsigned long long> rp_host;
    DevBuf<uint8_t> rp_ok;
    DevBuf<uint64_t> rp_bit;
    PinBuf<uint64_t> rp_hbit;
    // crc32c_repair_bytes: a host call's masks (the rest is crc32c_repair_items')
    DevBuf<uint8_t> rp_mask;
    PinBuf<uint8_t> rp_hmask;
    // crc32c_repair_headers: per header its candidates' count and scan; per
    // candidate its span (offset, length), record and CRC; the counters and
    // their pinned twin; a host call's verdicts, positions and lengths
    DevBuf<uint32_t> hd_cnt, hd_pre, hd_len, hd_crc, hd_lens;
    DevBuf<uint64_t> hd_off, hd_bit;
    DevBuf<mcrc_dev::HeaderRec> hd_recs;
    DevBuf<unsigned long long> hd_ctr;
    PinBuf<unsigned long long> hd_host;
    DevBuf<uint8_t> hd_ok;
    PinBuf<uint64_t> hd_hbit;
    PinBuf<uint32_t> hd_hlens;
    // crc32c_scrub_pages: the per-piece counts and scan of a repair list, the
    // list, a list length's pinned word, and a host call's flips of one round
    DevBuf<uint32_t> sc_cnt, sc_pre;
    DevBuf<uint64_t> sc_list, sc_foff, sc_fbit;
    DevBuf<uint8_t> sc_fby;
    PinBuf<uint32_t> sc_host;
    // ... with CRC32C_SCRUB_GAPS: the gap entries, and the merged list with them (the second list, a kind array per repair stage)
    DevBuf<uint64_t> sc_goffs, sc_moffs;
    DevBuf<uint32_t> sc_glens, sc_mlens;
    DevBuf<uint8_t> sc_mkind, sc_mikind;
    // ... with CRC32C_SCRUB_BYTES: a byte stage's bit count and its pinned twin (its masks: rp_mask)
    DevBuf<unsigned long long> sc_nbits;
    PinBuf<unsigned long long> sc_hbits;
    // crc32c_batch_ptrs: a device batch's rebased offsets, k_ptr_rebase's three
    // words and their pinned twin
    DevBuf<uint64_t> ptr_offs;
    DevBuf<unsigned long long> ptr_red;
    PinBuf<unsigned long long> ptr_hred;
    // pinned, device-mapped scratch of the host item-image calls
    MapBuf<> pin_stage, pin_ok;
    MapBuf<uint64_t> pin_offs;
    MapBuf<uint32_t> pin_crc;
};

// The device's shared scratch is the holder's on `st` until the end of its
// scope: taken in stream order, handed on by the busy event on every exit
// (sync: after `st` has drained, for calls whose results the host reads).
struct Lease {
    Device &d;
    hipStream_t st;
    bool sync;
    Lease(Device &dev, hipStream_t s, bool sync_first = false) : d(dev), st(s), sync(sync_first) { d.acquire(st); }
    Lease(const Lease &) = delete;
    ~Lease() {
        if (sync) (void)hipStreamSynchronize(st);
        d.release(st);
    }
};

std::mutex g_dev_mu;  // device discovery and first initialisation only
// Device state by HIP ordinal (every visible device; only gfx950 ones are
// ever initialised), and the library's device index -> HIP ordinal map: the
// gfx950 ordinals in order.  crc32c_gpu_count() is that map's size and
// crc32c_batch_multi's part g runs on HIP ordinal g_gfx[g], so a node whose
// first ordinals are other parts still shards over its gfx950 devices.
std::vector<std::unique_ptr<Device>> g_devs;
std::vector<int> g_gfx;
int g_nhip = -1;
// Initialised devices by ordinal, published once (release) after init_device:
// the per-call lookup reads them without g_dev_mu, so threads driving
// different devices (crc32c_batch_multi, IO threads on several GPUs) never
// serialise on a process-wide lock after the first call.
constexpr int kMaxDevices = 64;
std::atomic<Device *> g_ready[kMaxDevices];
std::atomic<int> g_ngfx_pub{-1};

// MCRC_DEBUG=1 in the environment: report the failing HIP call on stderr.
bool debug_on() {
    static const bool on = getenv("MCRC_DEBUG") != nullptr;
    return on;
}
#define HIP_OK(x)                                                                                  \
    do {                                                                                           \
        const hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) {                                                                    \
            if (debug_on()) fprintf(stderr, "mcrc: %s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return CRC32C_EHIP;                                                                    \
        }                                                                                          \
    } while (0)

bool is_gfx950(int ordinal) {
    hipDeviceProp_t p;
    return hipGetDeviceProperties(&p, ordinal) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

int init_device(Device &d, int id) {
    d.id = id;
    HIP_OK(hipSetDevice(id));
    hipDeviceProp_t p;
    HIP_OK(hipGetDeviceProperties(&p, id));
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) return CRC32C_ENODEV;
    d.cus = p.multiProcessorCount;
    // the table image of every table kernel: slice-by-4 tables replicated per
    // bank, the lane tree on 16-B granules, the half-item fold M_2048 and the
    // shifted last steps (crc32c_gf2.h build_lds_image_span at chunk 16)
    std::vector<uint32_t> img(mcrc::kImageK1Dwords);
    mcrc::build_lds_image_span(img.data(), mcrc_dev::kK1LaneBytes);
    std::vector<uint32_t> tab8(mcrc_dev::kTab8Dwords);  // [k][b]: the byte-wise table followed by k zero bytes
    mcrc::build_t0(tab8.data());
    for (uint32_t k = 1; k < 16; ++k) {
        const mcrc::Gf2Op zk = mcrc::Gf2Op::zeros(k);
        for (uint32_t b = 0; b < 256; ++b) tab8[256 * k + b] = zk.apply(tab8[b]);
    }
    const mcrc::Gf2Op z4k = mcrc::Gf2Op::zeros(mcrc_dev::kBlockBytes);  // tables 16..19: M_4096 by byte slice
    for (uint32_t k = 0; k < 4; ++k)
        for (uint32_t b = 0; b < 256; ++b) tab8[256 * (16 + k) + b] = z4k.apply(b << (8 * k));
    std::vector<uint32_t> xp(mcrc_dev::kXpowDwords);
    for (uint32_t j = 0; j < 1024; ++j) {
        xp[j] = mcrc::xpow8n(j);
        xp[1024 + j] = mcrc::xpow8n((uint64_t)j << 10);
        xp[2048 + j] = mcrc::xpow8n((uint64_t)j << 20);
    }
    for (uint32_t t = 0; t < mcrc_dev::kGridAlign; ++t) xp[mcrc_dev::kXpowInv + t] = mcrc::xpow8n_inv(t);
    for (uint32_t j = 0; j < 8; ++j) xp[mcrc_dev::kXpowL3 + j] = mcrc::xpow8n((uint64_t)j << 30);
    HIP_OK(hipMalloc(&d.img, img.size() * 4));
    HIP_OK(hipMemcpy(d.img, img.data(), img.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc(&d.tab8, tab8.size() * 4));
    HIP_OK(hipMemcpy(d.tab8, tab8.data(), tab8.size() * 4, hipMemcpyHostToDevice));
    // rows k (k < kSegpowLo) and kSegpowLo + j (x^(8 * 4096 * kSegpowLo j))
    // for every block shift in a 4 GiB span (a unit's shift: the blocks from
    // its end to the span's end)
    constexpr uint32_t lo = mcrc_dev::kSegpowLo;
    const uint32_t nhi = (uint32_t)((((1ull << 32) + 16) / mcrc_dev::kBlockBytes + 1 + lo - 1) / lo);
    std::vector<uint32_t> sp((lo + nhi) * 32);
    for (uint32_t k = 0; k < lo + nhi; ++k) {
        const uint64_t blocks = k < lo ? k : (uint64_t)lo * (k - lo);
        const uint32_t y = mcrc::xpow8n((uint64_t)mcrc_dev::kBlockBytes * blocks);
        for (uint32_t i = 0; i < 32; ++i) sp[k * 32 + i] = mcrc::mulmodp(0x80000000u >> i, y);
    }
    HIP_OK(hipMalloc(&d.segpow, sp.size() * 4));
    HIP_OK(hipMemcpy(d.segpow, sp.data(), sp.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc(&d.xpow, xp.size() * 4));
    HIP_OK(hipMemcpy(d.xpow, xp.data(), xp.size() * 4, hipMemcpyHostToDevice));
    d.xm128 = mcrc::xpow8n_inv(128);
    HIP_OK(hipMalloc(&d.zero, mcrc_dev::kZeroBytes));
    HIP_OK(hipMemset(d.zero, 0, mcrc_dev::kZeroBytes));
    HIP_OK(hipMalloc(&d.nbad, 2 * sizeof(unsigned long long)));
    HIP_OK(hipHostMalloc(&d.hbad, 2 * sizeof(unsigned long long), hipHostMallocDefault));
    HIP_OK(hipMalloc(&d.small_nbad, 16));
    HIP_OK(hipMemset(d.small_nbad, 0, 16));
    d.small_done = reinterpret_cast<uint32_t *>(d.small_nbad + 1);
    HIP_OK(hipMalloc(&d.k1_ctl, mcrc::kK1Slots * sizeof(mcrc_dev::K1Ctl)));
    HIP_OK(hipMemset(d.k1_ctl, 0, mcrc::kK1Slots * sizeof(mcrc_dev::K1Ctl)));
    HIP_OK(hipMalloc(&d.nfb, 2 * sizeof(uint32_t)));
    d.route = d.nfb + 1;
    for (hipStream_t *s : {&d.stream, &d.copy, &d.side}) HIP_OK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    for (hipEvent_t *e : {&d.fork, &d.join, &d.busy, &d.copied[0], &d.copied[1], &d.done[0], &d.done[1]})
        HIP_OK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    HIP_OK(hipEventCreate(&d.ev0));  // (the timed pair of a synchronous device batch)
    HIP_OK(hipEventCreate(&d.ev1));
    const void *k160[] = {
        (const void *)mcrc_dev::k_fixed<false, true>, (const void *)mcrc_dev::k_fixed<true, true>,
        (const void *)mcrc_dev::k_fixed<false, false>, (const void *)mcrc_dev::k_fixed<true, false>,
        (const void *)mcrc_dev::k_spans<false>, (const void *)mcrc_dev::k_spans<true>,
        (const void *)mcrc_dev::k_small<0>, (const void *)mcrc_dev::k_small<1>, (const void *)mcrc_dev::k_small<2>,
        (const void *)mcrc_dev::k_small<3>, (const void *)mcrc_dev::k_copy,
        (const void *)mcrc_dev::k_blocks<false, true>, (const void *)mcrc_dev::k_blocks<true, true>,
        (const void *)mcrc_dev::k_blocks<true, false>, (const void *)mcrc_dev::k_lines<0, true>,
        (const void *)mcrc_dev::k_lines<0, false>, (const void *)mcrc_dev::k_lines<1, true>,
        (const void *)mcrc_dev::k_lines<2, true>, (const void *)mcrc_dev::k_lines<3, true>,
    };
    for (const void *k : k160)
        HIP_OK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, mcrc_dev::kLdsImageK1Bytes));
    HIP_OK(hipDeviceSynchronize());  // (the memsets above, before a launch on a non-blocking stream)
    d.ok = true;
    return CRC32C_OK;
}

int ensure_devices() {  // (call with g_dev_mu held): the number of gfx950 devices
    if (g_nhip < 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) {
            (void)hipGetLastError();
            n = 0;
        }
        g_nhip = std::min(n, kMaxDevices);
        for (int i = 0; i < g_nhip; ++i) {
            g_devs.emplace_back(new Device());
            if (is_gfx950(i)) g_gfx.push_back(i);
        }
        g_ngfx_pub.store((int)g_gfx.size(), std::memory_order_release);
    }
    return (int)g_gfx.size();
}

int gfx_ordinal(int index) {  // library device index -> HIP ordinal (-1: none)
    std::lock_guard<std::mutex> lk(g_dev_mu);
    ensure_devices();
    return index >= 0 && index < (int)g_gfx.size() ? g_gfx[index] : -1;
}

// Device state for the calling thread's current HIP device.  After a
// device's first call this is hipGetDevice plus one acquire load.
int current_device(Device **out) {
    int id = 0;
    if (hipGetDevice(&id) != hipSuccess) return CRC32C_ENODEV;
    if (id >= 0 && id < kMaxDevices) {
        if (Device *r = g_ready[id].load(std::memory_order_acquire)) {
            *out = r;
            return CRC32C_OK;
        }
    }
    std::lock_guard<std::mutex> lk(g_dev_mu);
    ensure_devices();
    if (id < 0 || id >= g_nhip) return CRC32C_ENODEV;
    Device &d = *g_devs[id];
    if (!d.ok) {
        const int rc = init_device(d, id);
        if (rc != CRC32C_OK) return rc;
        g_ready[id].store(&d, std::memory_order_release);
    }
    *out = &d;
    return CRC32C_OK;
}

// [p, p + bytes) lies inside one device allocation (so no kernel read bounded
// by it can fault).  Memory the runtime cannot describe (e.g. host-registered
// or managed) is not checked.
bool device_range_ok(const void *p, uint64_t bytes) {
    hipDeviceptr_t lo = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&lo, &size, (hipDeviceptr_t)p) != hipSuccess || lo == nullptr) {
        (void)hipGetLastError();
        return true;
    }
    const uint64_t skip = (uint64_t)((const uint8_t *)p - (const uint8_t *)lo);
    return skip <= size && bytes <= size - skip;
}

const uint8_t *device_view_range(const void *p, uint64_t bytes);

// [p, p + bytes) can be the source of one DMA as it lies: device or managed
// memory, or host memory page-locked over the whole range.
bool is_pinned_or_device(const void *p, uint64_t bytes) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (at.type == hipMemoryTypeHost) return device_view_range(p, bytes) != nullptr;
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// The address a kernel reads host memory p at, when p is page-locked and
// mapped (crc32c_host_alloc, hipHostMalloc, crc32c_host_register); nullptr for
// pageable memory.
const uint8_t *device_view(const void *p) {
    hipPointerAttribute_t at;
    if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (at.type != hipMemoryTypeHost) return nullptr;
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, const_cast<void *>(p), 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return (const uint8_t *)dp;
}

// The device address of the whole host range [p, p + bytes) when every byte
// of it is page-locked and mapped as one contiguous range, else nullptr (the
// caller then stages the batch).  A caller may have registered only part of
// an arena, or pass a base_bytes past the end of its hipHostMalloc buffer: a
// kernel reading such a range in place would page-fault.  The runtime's
// record of the allocation or registration holding p must cover the range;
// where the runtime cannot describe it, both ends must map, to addresses
// bytes - 1 apart.
const uint8_t *device_view_range(const void *p, uint64_t bytes) {
    const uint8_t *dv = device_view(p);
    if (!dv || bytes <= 1) return dv;
    const uint8_t *h = (const uint8_t *)p;
    hipDeviceptr_t lo = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&lo, &size, (hipDeviceptr_t)p) == hipSuccess && lo) {
        // (the base comes back as the host or as the device address of the range)
        for (const uint8_t *q : {h, dv}) {
            const uint8_t *b = (const uint8_t *)lo;
            if (q >= b && (uint64_t)(q - b) <= size) return bytes <= size - (uint64_t)(q - b) ? dv : nullptr;
        }
        return nullptr;
    }
    (void)hipGetLastError();
    return device_view(h + bytes - 1) == dv + (bytes - 1) ? dv : nullptr;
}

}  // namespace
