// k_small.h -- batches of up to kSmallMax spans in one launch.
#pragma once

#include "k_spans.h"

namespace mcrc_dev {

// Small batches: one launch.  Up to kSmallMax spans, one 32-lane group per
// span, 32 spans per workgroup: the group reads the whole span [ph, Ea) in
// 4 KiB blocks anchored at Ea (no plan, no segments, no head fragment), reduces
// it to R, and its lanes compute Z from the span image's own tables
// (raw16 by dword steps, the x^(8n) multiplies) and emit.  The planned path's
// seven launches (count, scan, expand, span kernel x 2, final) cost ~80 us per
// call whatever the batch; a storage.c wbuf stamp (1007 images) or an IO-batch
// verify is one call of this kernel.

// Register after the 16 bytes of v from a zero register, on the span image's
// replicated slice-by-4 tables (this lane's copy).
__device__ __forceinline__ uint32_t raw16_img(Piece v, const LaneCtx &c) {
    uint32_t x = (uint32_t)v.lo;
    x = step4_next(x, (uint32_t)(v.lo >> 32), c);
    x = step4_next(x, (uint32_t)v.hi, c);
    x = step4_next(x, (uint32_t)(v.hi >> 32), c);
    return step4_next(x, 0u, c);
}

template <int MODE>
__global__ __launch_bounds__(1024) void k_small(SpanArgs a, const uint4 *__restrict__ img) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    load_tables(smem, img, kLdsImageK1Bytes);
    const uint32_t lane = threadIdx.x & 63u, li = lane & 31u;
    const LaneCtx c = make_lane_ctx(li);
    const uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
    const bool valid = i < a.n;
    ItemDesc it{a.base, 0u, 0u, false};
    if (valid) it = fetch_item<MODE>(a, i);
    const uint32_t len = it.sane ? it.len : 0u;
    const uint32_t t = tail_pad(it.p, len), eo = len + t;
    const uint32_t niters = len ? (eo + (uint32_t)((uintptr_t)it.p & 15u) + kBlockBytes - 1) / kBlockBytes : 0u;
    const uint32_t nmax = __builtin_amdgcn_readfirstlane(max(niters, (uint32_t)__shfl_xor(niters, 32, 64)));
    const uint4 *zero = zero_slot(a);
    uint32_t acc = 0;
    // block k + 1 is loaded before block k is reduced (two register sets)
    auto issue = [&](BlockWin &w, uint32_t k) {
        UnitDesc d;
        d.p = it.p;
        d.eo = eo;
        // (past the span: zeros; no tail mask: k_small's grid is 16-B, its Z has raw(F_t))
        d.nf = k < niters ? (niters << UnitDesc::kNitersShift) | UnitDesc::kValid : 0u;
        d.raw = 0;
        load_block(w, d, k, li, zero);
    };
    auto reduce = [&](const BlockWin &w, uint32_t k) {
        const uint32_t v = block_fold<0>(acc, true, w, c);
        if (k < niters) acc = v;
    };
    BlockWin w0, w1;
    if (nmax) issue(w0, 0);
    for (uint32_t k = 0; k < nmax; k += 2) {
        issue(w1, k + 1);
        reduce(w0, k);
        if (k + 1 >= nmax) break;
        issue(w0, k + 2);
        reduce(w1, k + 1);
    }
    const uint32_t R = group_reduce32_span(acc, lane);
    uint32_t nb = 0;
    if (valid) {
        // Z on k_small's own 16-B grid (its blocks keep F_t): M_{len+t}(~c ^ raw(F_h)) ^ raw(F_t)
        const uint32_t cin = MODE == 0 ? it.aux : 0u;
        uint32_t z = mulmodp_dev(~cin, a.xpow[t]);  // (len 0: R = 0, crc = c)
        if (len) {
            const uint32_t kh = (uint32_t)((uintptr_t)it.p & 15u);
            uint32_t y = ~cin;
            if (kh) y ^= raw16_img(shl_bytes(ld_piece(it.p - kh), 16 - kh), c);
            z = mulmodp_dev(y, xpow8_dev(a.xpow, (uint64_t)len + t));
            if (t) z ^= raw16_img(clear_below(ld_piece(it.p + len + t - 16), 16 - t), c);
        }
        if (MODE == 1) {
            const bool good = it.sane && R == (z ^ mulmodp_dev(~it.aux, a.xpow[t]));
            if (li == 0) a.ok[i] = good;
            nb = li == 0 && !good;
        } else {
            uint32_t v = R ^ z;
            if (t) v = mulmodp_dev(v, a.xpow[kXpowInv + t]);
            nb = li == 0 && emit<MODE>(a, i, ~v, it.sane, it.p, it.aux);  // (MODE 3: it.aux decides)
        }
    }
    // one atomic per wave with a bad span (all 160 KiB of LDS hold the tables,
    // so no workgroup-level sum as in count_bad)
    const uint64_t m = __ballot(nb != 0);
    if (m && lane == (uint32_t)(__ffsll((unsigned long long)m) - 1)) {
        atomicAdd(a.nbad, (unsigned long long)__popcll(m));
        // the add must be performed before this workgroup is counted done:
        // __syncthreads is a workgroup-scope release and does not wait for
        // another wave's outstanding global atomics, so without this fence
        // the last workgroup could read nbad before the add lands (a lost
        // count this call, a phantom one the next)
        __threadfence();
    }
    if (a.host_nbad) {
        // the last workgroup to finish hands the count to the host and leaves
        // the counters at zero for the next call: no memset before the launch
        // and no copy after it (two dispatches of a ~35 us synchronous call)
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            if (atomicAdd(a.done, 1u) == gridDim.x - 1) {
                __threadfence();
                *a.host_nbad = atomicExch(a.nbad, 0ull);
                atomicExch(a.done, 0u);
                __threadfence_system();
            }
        }
    }
}

}  // namespace mcrc_dev
