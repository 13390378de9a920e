// k1_timeline.hip -- dev tool (not part of the library): the timeline of one
// K1 launch, wave by wave.  It instantiates the product's loop
// (k_fixed_body, k_fixed.h) with a probe that stamps, per wave, the constant
// 100 MHz counter and the shader-clock counter at entry, after the table copy,
// every 8 steps and at exit (after the output stores have drained), plus the
// wave's XCC id and hardware id and the steps it ran (its claimed chunks
// included).  Both kernels get a counter block (K1Ctl) when the launch is long
// enough for the claimed tail; K1_TAIL=0 in the environment runs them without.
// Both run the product's order (kK1Order, kK1WindowScramble; k_consts.h) unless
// K1_ORDER (0 ranges, 1 window by step, 2 window by pass) and K1_SCRAMBLE (0 / 1:
// the windows dealt in launch order / scrambled) name another; the order that ran
// is printed.
// Lane 0 writes the stamps with plain vector stores.  The stamped launch's CRCs are checked equal to the product
// kernel's on the same batch.  Printed per item count:
//   - the product's and the stamped kernel's event times (what the stamps cost)
//   - wave, workgroup and XCD end percentiles (laid out like
//     profiles/r03_ablations/k1_tail_static_stamps.txt), the spread of the
//     wave ends inside a workgroup, each XCD's idle time before the launch's end
//   - the batch's bytes completed per 10 us bin as aggregate TB/s, the bulk
//     rate, and how much of the launch runs below it
//   - the shader clock per XCD (shader ticks per 100 MHz tick) over the bulk
//     and over the last 10 % of the launch
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I memcached_amd/csrc tools/k1_timeline.hip -o tools/k1_timeline
//   tools/k1_timeline [ITEMS ...]        (default: 1048576 4194304)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "crc32c_gf2.h"
#include "crc32c_kernels.hip"
#include "host_route.h"

using namespace mcrc_dev;

#define CHECK(x)                                                                       \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(2);                                                                   \
        }                                                                              \
    } while (0)

constexpr uint64_t kItemBytes = 4096, kStepBytes = 2 * kItemBytes;
constexpr uint32_t kEvery = 8;  // a stamp every 8 steps

// A wave's row: slot 0 entry, 1 after the table copy, 2 exit, 3 {hw id, xcc
// id}, 4 {steps run, 0}, 5 + j after step 8 (j + 1).
struct Stamp {
    uint64_t rt, sc;  // 100 MHz ticks, shader-clock ticks
};
constexpr uint32_t kFixedSlots = 5;

struct StampProbe {
    Stamp *row;
    uint32_t slots;  // of the row: nothing is written past it
    uint32_t lane;
    mutable uint64_t ran = 0;
    __device__ __forceinline__ void mark(uint32_t slot) const {
        const uint64_t rt = __builtin_amdgcn_s_memrealtime();
        const uint64_t sc = __builtin_amdgcn_s_memtime();
        if (lane == 0 && slot < slots) row[slot] = Stamp{rt, sc};
    }
    __device__ __forceinline__ void steps(uint64_t done) const {
        ran = done;
        if (done % kEvery == 0) mark(kFixedSlots + (uint32_t)(done / kEvery) - 1);
    }
    __device__ __forceinline__ void exit() const {
        __builtin_amdgcn_s_waitcnt(0);  // the out[] stores have drained
        mark(2);
        const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_ID
        const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
        if (lane == 0 && 4 < slots) row[3] = Stamp{hw, xcc}, row[4] = Stamp{ran, 0};
    }
};

template <int ORD, bool SCR>
__global__ __launch_bounds__(1024) void k_fixed_stamped(const uint8_t *__restrict__ base, uint64_t stride,
                                                        uint64_t nitems, const uint4 *__restrict__ img,
                                                        uint32_t *__restrict__ out, K1Ctl *__restrict__ ctl, Stamp *st,
                                                        uint32_t slots) {
    const uint32_t wid = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const StampProbe probe{st + (uint64_t)wid * slots, slots, threadIdx.x & 63u};
    probe.mark(0);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    load_tables(smem, img, kLdsImageK1Bytes);
    probe.mark(1);
    k_fixed_body<false, true, StampProbe, (K1Order)ORD, SCR>(base, stride, nitems, img, nullptr, out, blockDim.x, ctl, probe);
}
// (the product's kernel, k_fixed, in the same order)
template <int ORD, bool SCR>
__global__ __launch_bounds__(1024) void k_fixed_plain(const uint8_t *__restrict__ base, uint64_t stride, uint64_t nitems,
                                                      const uint4 *__restrict__ img, uint32_t *__restrict__ out,
                                                      K1Ctl *__restrict__ ctl) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    load_tables(smem, img, kLdsImageK1Bytes);
    k_fixed_body<false, true, K1NoProbe, (K1Order)ORD, SCR>(base, stride, nitems, img, nullptr, out, blockDim.x, ctl,
                                                            K1NoProbe{});
}
struct OrderKernels {
    int order;
    bool scramble;
    const char *name;
    const void *stamped, *plain;
};
#define ORDER_KERNELS(O, S, NAME) \
    OrderKernels { O, S, NAME, (const void *)k_fixed_stamped<O, S>, (const void *)k_fixed_plain<O, S> }
static const OrderKernels kOrders[] = {
    ORDER_KERNELS(0, true, "ranges, dealt scrambled"),
    ORDER_KERNELS(1, false, "window by step, windows in launch order"),
    ORDER_KERNELS(1, true, "window by step, windows dealt scrambled"),
    ORDER_KERNELS(2, false, "window by pass, windows in launch order"),
    ORDER_KERNELS(2, true, "window by pass, windows dealt scrambled"),
};

__global__ void fill(uint32_t *p, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t z = (i + 1) * 0x9e3779b97f4a7c15ull;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        p[i] = (uint32_t)(z ^ (z >> 31));
    }
}

template <typename F>
static void time_stats(F launch, int reps, float *med, float *mn, float *mx) {
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    std::vector<float> t;
    for (int r = 0; r < reps; ++r) {
        CHECK(hipEventRecord(a, 0));
        launch();
        CHECK(hipEventRecord(b, 0));
        CHECK(hipEventSynchronize(b));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, a, b));
        t.push_back(ms);
    }
    std::sort(t.begin(), t.end());
    *med = t[t.size() / 2], *mn = t.front(), *mx = t.back();
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
}

static double pct(const std::vector<double> &sorted, double p) {
    return sorted[(size_t)std::min<double>(sorted.size() - 1, p / 100.0 * (sorted.size() - 1) + 0.5)];
}

struct Wave {
    uint32_t xcc, wg;
    uint64_t nsteps;
    std::vector<Stamp> s;  // the table-copy stamp, the step stamps, the exit stamp: in time order
    std::vector<uint64_t> done;  // steps completed at each of them
    double t_entry, t_tables, t_end;  // us since the first entry
};

static void analyse(uint64_t n, int grid, const std::vector<Stamp> &st, uint32_t slots, bool claimed, const OrderKernels &ok) {
    const uint64_t nw = (uint64_t)grid * 16, ngroups = (n + 1) / 2, cg = (ngroups + nw - 1) / nw;
    const K1Order run = k1_order_for((K1Order)ok.order, cg);
    uint64_t t0 = ~0ull;
    for (uint64_t w = 0; w < nw; ++w) t0 = std::min(t0, st[w * slots].rt);
    auto us = [&](uint64_t rt) { return (double)(rt - t0) / 100.0; };
    std::vector<Wave> wv(nw);
    double span = 0;
    for (uint64_t w = 0; w < nw; ++w) {
        const Stamp *r = &st[w * slots];
        Wave &x = wv[w];
        x.wg = (uint32_t)(w / 16);
        x.xcc = (uint32_t)r[3].sc & 15u;
        // K1's walk (k1_walk, k_consts.h): a range is cut at the batch's end, a window's wave runs all its steps
        const K1Walk wk = k1_walk(run, ok.scramble, (uint32_t)(w / 16), (uint32_t)(w % 16), (uint32_t)grid, 16, cg);
        const uint64_t g0 = wk.first, g1 = run == kK1OrderRanges ? std::min(wk.end, ngroups) : g0 + cg;
        // (with the claimed tail: what the wave counted, whole passes)
        x.nsteps = claimed ? r[4].rt : g0 < ngroups ? g1 - g0 : 0;
        x.t_entry = us(r[0].rt), x.t_tables = us(r[1].rt), x.t_end = us(r[2].rt);
        x.s.push_back(r[1]), x.done.push_back(0);
        for (uint64_t d = kEvery; d <= x.nsteps / 4 * 4 && kFixedSlots + d / kEvery - 1 < slots; d += kEvery)
            x.s.push_back(r[kFixedSlots + d / kEvery - 1]), x.done.push_back(d);
        x.s.push_back(r[2]), x.done.push_back(x.nsteps);
        span = std::max(span, x.t_end);
    }
    auto sorted = [](std::vector<double> v) {
        std::sort(v.begin(), v.end());
        return v;
    };
    std::vector<double> e, b, c, ends;
    for (auto &x : wv) e.push_back(x.t_entry), c.push_back(x.t_tables - x.t_entry), ends.push_back(x.t_end);
    e = sorted(e), c = sorted(c), ends = sorted(ends);
    if (claimed) {
        std::vector<double> ns;
        for (auto &x : wv) ns.push_back((double)x.nsteps);
        ns = sorted(ns);
        const K1Tail tl = k1_tail_split(ngroups, nw);
        printf("\nn %llu: claimed tail: %llu static steps per wave, %llu chunks of %u steps; steps run per wave p0/p10/p50/p90/p100 "
               "%.0f/%.0f/%.0f/%.0f/%.0f",
               (unsigned long long)n, (unsigned long long)tl.cg_s, (unsigned long long)tl.nchunks, (unsigned)kK1TailSteps,
               ns.front(), pct(ns, 10), pct(ns, 50), pct(ns, 90), ns.back());
        for (uint32_t xc = 0; xc < 16; ++xc) {
            double sum = 0;
            size_t cnt = 0;
            for (auto &x : wv)
                if (x.xcc == xc) sum += (double)x.nsteps, ++cnt;
            if (cnt) printf("%s xcc %u %.1f", xc ? "," : "; mean per XCD:", xc, sum / cnt);
        }
    }
    printf("\nn %llu: span %.1f us; grid %d x 16 waves, %llu steps per wave; wave start p0/p50/p100 %.1f/%.1f/%.1f us; "
           "table copy p50/p100 %.1f/%.1f us\n",
           (unsigned long long)n, span, grid, (unsigned long long)cg, e.front(), pct(e, 50), e.back(), pct(c, 50),
           c.back());
    printf("wave end p0 %.1f p1 %.1f p10 %.1f p50 %.1f p90 %.1f p99 %.1f p100 %.1f us\n", ends.front(), pct(ends, 1),
           pct(ends, 10), pct(ends, 50), pct(ends, 90), pct(ends, 99), ends.back());
    double xend[16] = {0}, xmean = 0;
    int nx = 0;
    for (uint32_t xc = 0; xc < 16; ++xc) {
        std::vector<double> v;
        for (auto &x : wv)
            if (x.xcc == xc) v.push_back(x.t_end);
        if (v.empty()) continue;
        v = sorted(v);
        xend[xc] = v.back(), xmean += v.back(), ++nx;
        printf("  xcc %u: %zu waves, end p0 %.1f p50 %.1f p100 %.1f us; idle before the launch's end %.1f us\n", xc,
               v.size(), v.front(), pct(v, 50), v.back(), span - v.back());
    }
    xmean /= nx;
    printf("XCD end (last wave): mean %.1f us = %.3f of the span\n", xmean, xmean / span);
    std::vector<double> wgend(grid, 0), wgfirst(grid, 1e30), spread;
    for (auto &x : wv) wgend[x.wg] = std::max(wgend[x.wg], x.t_end), wgfirst[x.wg] = std::min(wgfirst[x.wg], x.t_end);
    for (int g = 0; g < grid; ++g) spread.push_back(wgend[g] - wgfirst[g]);
    wgend = sorted(wgend), spread = sorted(spread);
    printf("workgroup end (last wave) p0 %.1f p10 %.1f p50 %.1f p90 %.1f p100 %.1f us\n", wgend.front(), pct(wgend, 10),
           pct(wgend, 50), pct(wgend, 90), wgend.back());
    printf("wave ends inside a workgroup, last - first: p0 %.1f p50 %.1f p90 %.1f p100 %.1f us\n", spread.front(),
           pct(spread, 50), pct(spread, 90), spread.back());

    // bytes completed per 10 us bin: a wave's bytes between two stamps spread
    // evenly over the time between them
    const double bin = 10.0;
    const size_t nb = (size_t)(span / bin) + 1;
    std::vector<double> by(nb, 0.0);
    for (auto &x : wv)
        for (size_t i = 1; i < x.s.size(); ++i) {
            const double a = us(x.s[i - 1].rt), z = us(x.s[i].rt), bytes = (double)(x.done[i] - x.done[i - 1]) * kStepBytes;
            if (bytes == 0) continue;
            if (z <= a) {
                by[std::min(nb - 1, (size_t)(a / bin))] += bytes;
                continue;
            }
            for (size_t k = (size_t)(a / bin); k < nb && k * bin < z; ++k) {
                const double lo = std::max(a, k * bin), hi = std::min(z, (k + 1) * bin);
                if (hi > lo) by[k] += bytes * (hi - lo) / (z - a);
            }
        }
    printf("aggregate TB/s per 10 us bin (ten bins a line; the last bin is %.1f us long):\n", span - (nb - 1) * bin);
    std::vector<double> rate(nb);
    for (size_t k = 0; k < nb; ++k) {
        const double len = k + 1 < nb ? bin : std::max(span - k * bin, 1e-9);
        rate[k] = by[k] / (len * 1e-6) / 1e12;
        if (k % 10 == 0) printf("  %6.0f us:", k * bin);
        printf(" %5.2f", rate[k]);
        if (k % 10 == 9 || k + 1 == nb) printf("\n");
    }
    // the bulk rate: the median bin between 20 % and 70 % of the span
    std::vector<double> mid(rate.begin() + nb / 5, rate.begin() + std::max(nb / 5 + 1, nb * 7 / 10));
    const double bulk = pct(sorted(mid), 50);
    size_t head = 0, tail = nb;
    while (head < nb && rate[head] < 0.95 * bulk) ++head;
    while (tail > head && rate[tail - 1] < 0.95 * bulk) --tail;
    double lost_head = 0, lost_tail = 0;
    for (size_t k = 0; k < nb; ++k) {
        const double len = k + 1 < nb ? bin : span - k * bin;
        const double l = std::max(0.0, bulk - rate[k]) * len;
        if (k < head) lost_head += l;
        if (k >= tail) lost_tail += l;
    }
    const double total = (double)n * kItemBytes;
    printf("bulk rate (median bin of 20-70 %% of the span) %.2f TB/s; the launch's mean %.2f TB/s = %.3f of the bulk\n", bulk,
           total / (span * 1e-6) / 1e12, total / (span * 1e-6) / 1e12 / bulk);
    printf("below 0.95 of the bulk rate: the first %.0f us (%.1f %% of the span) and the last %.0f us (%.1f %%); the time the "
           "missing bytes would take at the bulk rate: start %.1f us (%.1f %%), end %.1f us (%.1f %%)\n",
           head * bin, head * bin / span * 100, span - tail * bin, (span - tail * bin) / span * 100, lost_head / bulk,
           lost_head / bulk / span * 100, lost_tail / bulk, lost_tail / bulk / span * 100);

    // the shader clock per XCD: shader ticks per 100 MHz tick, summed over the
    // XCD's waves, from the table copy to the last stamp before 90 % of the
    // span (bulk) and from there to the exit (the last 10 %)
    printf("shader clock per XCD (MHz = shader ticks per 100 MHz tick x 100), bulk | last 10 %% of the span:\n");
    for (uint32_t xc = 0; xc < 16; ++xc) {
        double bs = 0, br = 0, ts = 0, tr = 0;
        size_t ntail = 0;
        for (auto &x : wv) {
            if (x.xcc != xc || x.s.size() < 2) continue;
            size_t cut = 0;
            for (size_t i = 0; i < x.s.size(); ++i)
                if (us(x.s[i].rt) <= 0.9 * span) cut = i;
            bs += (double)(x.s[cut].sc - x.s[0].sc), br += (double)(x.s[cut].rt - x.s[0].rt);
            if (cut + 1 < x.s.size()) {
                ts += (double)(x.s.back().sc - x.s[cut].sc), tr += (double)(x.s.back().rt - x.s[cut].rt);
                ++ntail;
            }
        }
        if (br == 0) continue;
        printf("  xcc %u: %7.1f MHz |", xc, bs / br * 100);
        if (tr > 0) printf(" %7.1f MHz (%zu waves still running)\n", ts / tr * 100, ntail);
        else printf(" (no wave left)\n");
    }
}

int main(int argc, char **argv) {
    std::vector<uint64_t> sizes;
    for (int i = 1; i < argc; ++i) sizes.push_back(strtoull(argv[i], nullptr, 0));
    if (sizes.empty()) sizes = {1ull << 20, 4ull << 20};
    const int reps = 30;
    hipDeviceProp_t p;
    CHECK(hipGetDeviceProperties(&p, 0));
    const int cus = p.multiProcessorCount;
    const bool want_tail = !(getenv("K1_TAIL") && atoi(getenv("K1_TAIL")) == 0);
    const int want_order = getenv("K1_ORDER") ? atoi(getenv("K1_ORDER")) : (int)kK1Order;
    const bool want_scr = want_order == 0 || (getenv("K1_SCRAMBLE") ? atoi(getenv("K1_SCRAMBLE")) != 0 : kK1WindowScramble);
    const OrderKernels *ok = nullptr;
    for (const OrderKernels &k : kOrders)
        if (k.order == want_order && k.scramble == want_scr) ok = &k;
    if (!ok) {
        fprintf(stderr, "K1_ORDER must be 0, 1 or 2\n");
        return 2;
    }
    printf("device %s  CUs %d  K1 lockstep round: %u steps; claimed tail %s (from %u steps per wave, 1/%u of a range, chunks of "
           "%u steps)\n",
           p.gcnArchName, cus, (unsigned)kK1RoundSteps, want_tail ? "on" : "off", (unsigned)kK1TailMinSteps,
           1u << kK1TailShift, (unsigned)kK1TailSteps);
    printf("K1 order: %s%s, in launches of at least %u steps per wave (shorter ones: ranges)\n", ok->name,
           want_order == (int)kK1Order && (want_order == 0 || want_scr == kK1WindowScramble) ? " (the product's)" : "",
           (unsigned)kK1RoundsMinSteps);
    K1Ctl *dctl;
    CHECK(hipMalloc(&dctl, sizeof(K1Ctl)));
    CHECK(hipMemset(dctl, 0, sizeof(K1Ctl)));
    const uint64_t nmax = *std::max_element(sizes.begin(), sizes.end());
    uint8_t *d;
    uint32_t *out, *out_ref;
    CHECK(hipMalloc(&d, nmax * kItemBytes));
    CHECK(hipMalloc(&out, nmax * 4));
    CHECK(hipMalloc(&out_ref, nmax * 4));
    fill<<<4096, 256>>>((uint32_t *)d, nmax * kItemBytes / 4);
    std::vector<uint32_t> img(mcrc::kImageK1Dwords);
    mcrc::build_lds_image_span(img.data(), kK1LaneBytes);
    uint4 *dimg;
    CHECK(hipMalloc(&dimg, img.size() * 4));
    CHECK(hipMemcpy(dimg, img.data(), img.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipFuncSetAttribute(ok->plain, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsImageK1Bytes));
    CHECK(hipFuncSetAttribute(ok->stamped, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsImageK1Bytes));
    const uint64_t stride = kItemBytes;
    for (const uint64_t n : sizes) {
        const int grid = mcrc::grid_for(cus, n);
        const uint64_t nw = (uint64_t)grid * 16, cg = ((n + 1) / 2 + nw - 1) / nw;
        // (a wave that claims runs more steps than cg: rows of twice that, and
        // nothing is written past a row)
        const uint32_t slots = kFixedSlots + (uint32_t)(2 * cg / kEvery) + 1;
        K1Ctl *ctl = want_tail && cg >= kK1TailMinSteps ? dctl : nullptr;
        Stamp *st;
        CHECK(hipMalloc(&st, nw * slots * sizeof(Stamp)));
        CHECK(hipMemset(st, 0, nw * slots * sizeof(Stamp)));
        auto product = [&] {
            void *args[] = {(void *)&d, (void *)&stride, (void *)&n, (void *)&dimg, (void *)&out_ref, (void *)&ctl};
            CHECK(hipLaunchKernel(ok->plain, dim3(grid), dim3(1024), args, kLdsImageK1Bytes, 0));
        };
        auto stamped = [&] {
            void *args[] = {(void *)&d,   (void *)&stride, (void *)&n,  (void *)&dimg,
                            (void *)&out, (void *)&ctl,    (void *)&st, (void *)&slots};
            CHECK(hipLaunchKernel(ok->stamped, dim3(grid), dim3(1024), args, kLdsImageK1Bytes, 0));
        };
        // clock settle: 300 ms of back-to-back product launches
        const auto c0 = std::chrono::steady_clock::now();
        while (std::chrono::steady_clock::now() - c0 < std::chrono::milliseconds(300)) {
            for (int i = 0; i < 10; ++i) product();
            CHECK(hipDeviceSynchronize());
        }
        const double gb = (double)n * kItemBytes;
        for (int round = 0; round < 2; ++round) {
            float med, mn, mx;
            time_stats(product, reps, &med, &mn, &mx);
            printf("round %d n %llu k_fixed: median %.4f ms  min %.4f  max %.4f  (%.1f %% of 8 TB/s at median)\n", round,
                   (unsigned long long)n, med, mn, mx, gb / (med * 1e-3) / 8e12 * 100);
            CHECK(hipMemset(out, 0, n * 4));
            time_stats(stamped, reps, &med, &mn, &mx);
            printf("round %d n %llu stamped: median %.4f ms  min %.4f  max %.4f  (%.1f %% of 8 TB/s at median)\n", round,
                   (unsigned long long)n, med, mn, mx, gb / (med * 1e-3) / 8e12 * 100);
        }
        std::vector<uint32_t> h(n), href(n);
        CHECK(hipMemcpy(h.data(), out, n * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(href.data(), out_ref, n * 4, hipMemcpyDeviceToHost));
        const bool same = memcmp(h.data(), href.data(), n * 4) == 0;
        printf("n %llu: stamped CRCs %s the product kernel's\n", (unsigned long long)n, same ? "equal" : "DIFFER FROM");
        std::vector<Stamp> hs(nw * slots);
        CHECK(hipMemcpy(hs.data(), st, hs.size() * sizeof(Stamp), hipMemcpyDeviceToHost));  // (the last stamped launch)
        analyse(n, grid, hs, slots, ctl != nullptr, *ok);
        fflush(stdout);
        CHECK(hipFree(st));
        if (!same) return 1;
    }
    CHECK(hipFree(d));
    CHECK(hipFree(out));
    CHECK(hipFree(out_ref));
    return 0;
}
