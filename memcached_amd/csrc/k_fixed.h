// k_fixed.h -- K1: equal 4 KiB, 16-B aligned items at a fixed stride (the lane
// layout and its algebra: k_common.h, "K1's lane layout").
#pragma once

#include "k_common.h"

namespace mcrc_dev {

// Half an item's pieces for one lane (pieces 4 q .. 4 q + 3 of half q).
struct K1Half {
    uint4 d[4];
    uint32_t cin;  // (half 0) the item's initial CRC
};
// The value of half Q: its four chains, each ended by its shifted last step
// (M_1536, M_1024, M_512, plain: the half's pieces stand 512 (3 - k) from its
// end); the item's lane value is M_2048(u_0) ^ u_1 (half0 / part0 of k_fixed;
// K4 and K5 form it over a whole window: k1_lane_value, k_window.h).
__device__ __forceinline__ uint32_t k1_half_value(const K1Half &r, const LaneCtx &c) {
    constexpr uint32_t kShift[3] = {kAuxShift0, kAuxShift1, kAuxShift2};
    uint32_t x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = r.d[k].x;
#pragma unroll
    for (int i = 1; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = step4_next(x[k], dw4(r.d[k], i), c);
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = k < 3 ? step4_last_shifted(x[k], kShift[k]) : step4_next(x[k], 0u, c);
    return xor3(x[0], x[1], x[2]) ^ x[3];
}

// A round's end: a bare workgroup barrier.  It carries no data, so unlike
// __syncthreads() it has no fence, whose vmcnt(0) would drain the prefetched
// half-steps; the sched_barriers keep the loads and chains on their sides.
__device__ __forceinline__ void k1_round_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// The probe policy of k_fixed_body: points of a wave's life.  The product
// passes this no-op, which compiles away; tools/k1_timeline.hip passes one
// that stamps the clocks (its exit() drains the output stores first).
struct K1NoProbe {
    __device__ __forceinline__ void steps(uint64_t /*done*/) const {}  // at the bottom of a 4-step pass
    __device__ __forceinline__ void exit() const {}
};

// K1's body behind the table copy (k_fixed below is the product's kernel
// around it).  The copy and the read of blockDim.x (nthreads) stay in the
// kernel: a function is optimised on its own before it is inlined, and
// blockDim.x read in here no longer folded to the dispatch packet's field
// (a select between two loads instead, 9 instructions more per kernel).
// NT: non-temporal loads, for a 128-B aligned base and stride (every line
// whole in one item); otherwise the default policy, so that a line two
// neighbouring items share is not fetched twice (the ldh lambda below).
template <bool CRCIN, bool NT, class Probe>
__device__ __forceinline__ void k_fixed_body(const uint8_t *__restrict__ base, uint64_t stride, uint64_t nitems,
                                             const uint4 *__restrict__ img, const uint32_t *__restrict__ crc_in,
                                             uint32_t *__restrict__ out, uint32_t nthreads,
                                             const Probe &probe) {
    constexpr uint32_t IPW = 2;  // items per wave and step
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t li = lane & 31u;
    const uint32_t g = lane >> 5;
    const LaneCtx c = make_lane_ctx(li);
    const uint64_t waves = nthreads >> 6;
    const uint64_t gstep = gridDim.x * waves;
    const uint64_t ngroups = (nitems + IPW - 1) / IPW;
    // wave-uniform (SGPR) group index: the loop exits are then scalar
    // branches, and the waitcnt pass sees one path into the loop header (a
    // divergent exit merged an un-waited path there and forced vmcnt(0),
    // which drained the prefetched step).
    uint64_t grp = __builtin_amdgcn_readfirstlane(blockIdx.x * (uint32_t)waves + (threadIdx.x >> 6));
    // the ranges dealt to the waves in a scrambled order: wave w takes range
    // (w * 65521) mod W (65521 is prime: a bijection unless it divides W), so
    // a CU's 16 waves stream ranges far apart rather than 16 neighbouring
    // MiB: -0.6 % at 1 and 4 Mi items in every round
    // (profiles/r04_ablations/k1_range_order_ab.txt)
    if (gstep % 65521u) grp = (grp * 65521u) % gstep;
    // wave w takes the contiguous groups [w cg, (w + 1) cg): 1.0-1.4 % faster
    // than the grid-stride order at 1 Mi items, 0.6-3.7 % at 4 Mi, on two
    // boxes (profiles/r04_ablations/k1_chunk_and_census_ab.txt,
    // k1_item_order_ab.txt); a range per workgroup with its waves interleaved
    // was 4.5 % slower
    const uint64_t cg = (ngroups + gstep - 1) / gstep;
    const uint64_t gend = min((grp + 1) * cg, ngroups);
    grp *= cg;
    // Lockstep rounds: the barriers this wave still owes its workgroup, from
    // cg alone (k1_rounds, k_consts.h), so every wave of the grid starts with
    // the same count -- also a wave whose range is empty or cut short at the
    // batch's end.  It arrives once per kK1RoundSteps steps of its 4-step loop
    // while it owes an arrival (never in a launch too short for rounds) and
    // makes up the rest behind its last store: every wave executes exactly
    // k1_rounds(cg) barriers on every path, and nothing relies on ended waves
    // being dropped from the barrier.
    uint64_t owed = k1_rounds(cg, kK1RoundSteps);
    const bool busy = grp < ngroups;  // (wave-uniform) an empty range only pays its barriers
    const uint64_t glast = gend - 1;
    auto item_of = [&](uint64_t gi) { return gi * IPW + g; };

    // The loads run three half-steps ahead: a ring of four half-buffers (the
    // registers of two whole steps), so while one half is checksummed the
    // next three (12 KiB per wave) are in flight.  Uniform step base +
    // per-lane offset: no 64-bit VGPR address math at the top of a step.  A
    // wave's last prefetches run past its last group; they read the table
    // image instead (in L2 since every workgroup copied it; their results are
    // not used): re-reading the wave's last group fetched it from HBM again
    // (non-temporal loads), 0.7 % of the launch's bytes, and clamping every
    // wave to the batch's last group made 4096 waves read the same 8 KiB at
    // the end of the launch.  The sched_barrier keeps the loads where they
    // are issued: left alone, the scheduler sinks them into the chains and
    // the next half waits on loads issued moments before.
    auto ldh = [&](K1Half &r, uint64_t gi, int q) {
        const bool real = gi < gend;  // (wave-uniform)
        const uint64_t gu = real ? gi : glast;
        const uint64_t first = gu * IPW;
        const uint8_t *wb = real ? base + first * stride : reinterpret_cast<const uint8_t *>(img);
        const uint32_t gl = first + g < nitems ? g : (uint32_t)(nitems - 1 - first);
        // crc_in first: it is consumed before the first chain step, and
        // vmcnt counts in issue order
        if (q == 0) {
            if constexpr (CRCIN) r.cin = crc_in[first + gl];
            else r.cin = 0u;
        }
        const uint32_t loff = (real ? gl * (uint32_t)stride : g * kK1Bytes) + li * kK1LaneBytes + 4u * kK1Piece * (uint32_t)q;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            r.d[k] = NT ? ld16_nt(wb + loff + k * kK1Piece) : ld16((gbyte *)(wb + loff + k * kK1Piece));
        __builtin_amdgcn_sched_barrier(0);
    };
    // lane 0 XORs ~crc_in into the item's first dword (a register seeded
    // with ~crc_in, crc32c.c:166)
    auto half0 = [&](K1Half &m) {
        if (li == 0) m.d[0].x ^= ~m.cin;
        return apply_op<4>(kAuxSpanFold, k1_half_value(m, c));
    };
    auto part0 = [&](uint32_t u0, K1Half &m1) {
        return reduce_level<0>(u0 ^ k1_half_value(m1, c), (lane & 1u) == 0u);
    };
    K1Half h0, h1, h2, h3;
    // Step k's halves live in h0/h1 (k even) or h2/h3 (k odd).  Before step k
    // is checksummed, its two halves and step k + 1's first are issued; each
    // half's checksum is preceded by the issue of the half three later.
    // (even step k at grp: h0/h1 -> issue h3 (k+1, B), h0 (k+2, A))
    auto step_even = [&](uint64_t s) {
        ldh(h3, s + 1, 1);
        const uint32_t u0 = half0(h0);
        ldh(h0, s + 2, 0);
        return part0(u0, h1);
    };
    auto step_odd = [&](uint64_t s) {
        ldh(h1, s + 1, 1);
        const uint32_t u0 = half0(h2);
        ldh(h2, s + 2, 0);
        return part0(u0, h3);
    };
    if (busy) {
        const uint64_t nsteps = gend - grp;  // (<= cg)
        ldh(h0, grp, 0);
        ldh(h1, grp, 1);
        ldh(h2, grp + 1, 0);
        // One exit, at the bottom of each loop: a break between the halves would
        // give the loop header a second (un-waited) predecessor, and the waitcnt
        // pass would then drain every prefetched load there.
        uint64_t k = 0;
        for (; k + 4 <= nsteps; k += 4) {
            const uint32_t va = step_even(grp);
            const uint32_t vb = step_odd(grp + 1);
            const uint32_t vab = group_pair_level1(va, vb, lane);
            const uint32_t vc = step_even(grp + 2);
            const uint32_t vd = step_odd(grp + 3);
            const uint32_t raw = group_reduce32_quad_span(vab, group_pair_level1(vc, vd, lane), lane);
            const uint64_t item = item_of(grp + (li & 3u));
            if (li < 4 && item < nitems) out[item] = ~raw;
            grp += 4;
            // (the three half-steps in flight stay in flight across it)
            if ((k + 4) % kK1RoundSteps == 0 && owed) {
                k1_round_barrier();
                --owed;
            }
            probe.steps(k + 4);
        }
        for (; k + 2 <= nsteps; k += 2) {
            const uint32_t va = step_even(grp);
            const uint32_t vb = step_odd(grp + 1);
            const uint32_t raw = group_reduce32_pair_span(va, vb, lane);
            const uint64_t item = item_of(li == 0 ? grp : grp + 1);
            if (li < 2 && item < nitems) out[item] = ~raw;
            grp += 2;
        }
        if (nsteps & 1) {
            const uint32_t raw = group_reduce32_single_span(step_even(grp), lane);
            const uint64_t item = item_of(grp);
            if (li == 0 && item < nitems) out[item] = ~raw;
        }
    }
    for (; owed; --owed) k1_round_barrier();
    probe.exit();
}

template <bool CRCIN, bool NT>
__global__ __launch_bounds__(1024) void k_fixed(const uint8_t *__restrict__ base, uint64_t stride,
                                                uint64_t nitems, const uint4 *__restrict__ img,
                                                const uint32_t *__restrict__ crc_in,
                                                uint32_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    load_tables(smem, img, kLdsImageK1Bytes);
    k_fixed_body<CRCIN, NT>(base, stride, nitems, img, crc_in, out, blockDim.x, K1NoProbe{});
}

}  // namespace mcrc_dev
