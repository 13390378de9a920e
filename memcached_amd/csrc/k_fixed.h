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
    // at the bottom of a 4-step pass: the steps the wave has run, its claimed
    // chunks included (a cut chunk counts as a whole pass)
    __device__ __forceinline__ void steps(uint64_t /*done*/) const {}
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
// ctl: null, or the launch's counters (K1Ctl, k_consts.h): the launch then
// runs k1_tail_split's static part in the loop below and claims the pool's
// chunks behind it ("The claimed tail").
// ORD, SCR: the order of the static part (K1Order, k_consts.h) in a launch with
// lockstep rounds, and whether its windows are dealt scrambled; the product's
// are kK1Order and kK1WindowScramble, the tools instantiate the others.
template <bool CRCIN, bool NT, class Probe, K1Order ORD = kK1Order, bool SCR = kK1WindowScramble>
__device__ __forceinline__ void k_fixed_body(const uint8_t *__restrict__ base, uint64_t stride, uint64_t nitems,
                                             const uint4 *__restrict__ img, const uint32_t *__restrict__ crc_in,
                                             uint32_t *__restrict__ out, uint32_t nthreads, K1Ctl *__restrict__ ctl,
                                             const Probe &probe) {
    constexpr uint32_t IPW = 2;  // items per wave and step
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t li = lane & 31u;
    const uint32_t g = lane >> 5;
    const LaneCtx c = make_lane_ctx(li);
    const uint64_t waves = nthreads >> 6;
    const uint64_t gstep = gridDim.x * waves;
    const uint64_t ngroups = (nitems + IPW - 1) / IPW;
    // (with a claimed tail: the static part's full ranges of cg_s steps)
    const bool tail = ctl != nullptr;  // (a kernel argument: wave-uniform)
    const K1Tail tl = tail ? k1_tail_split(ngroups, gstep) : K1Tail{0, 0, 0};
    const uint64_t cg = tail ? tl.cg_s : (ngroups + gstep - 1) / gstep;
    // The order (k1_walk, k_consts.h).  A launch with
    // lockstep rounds runs ORD, the product a window per workgroup read pass by
    // pass: its waves stay within a pass of each other, so the workgroup reads
    // 512 KiB of neighbouring addresses together, 32 KiB per wave: 2.6 % faster
    // than the ranges at 1 Mi items, 3.3 % at 4 Mi, in every round
    // (profiles/k1_order_ab.jsonl; the bulk rate 7.30 against 6.99 TB/s,
    // profiles/k1_order_timeline.txt).  A launch too short for rounds streams a
    // contiguous range per wave, the ranges dealt scrambled so that a CU's 16
    // waves read far apart: its waves drift, and what they would share is then
    // read microseconds apart.
    // wave-uniform (SGPR) group index: the loop exits are then scalar
    // branches, and the waitcnt pass sees one path into the loop header (a
    // divergent exit merged an un-waited path there and forced vmcnt(0),
    // which drained the prefetched step).
    const uint32_t wslot = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const K1Order ord = k1_order_for(ORD, cg);
    const K1Walk wk = k1_walk(ord, SCR, blockIdx.x, wslot, gridDim.x, (uint32_t)waves, cg);
    uint64_t grp = wk.first;
    // (the strides between a pass's steps and between passes: constants where
    // the build's orders leave no choice)
    const uint64_t ss = ORD == kK1OrderWindowStep ? wk.sstep : 1;
    const uint64_t ps = ORD == kK1OrderRanges ? 4 : wk.pstep;
    uint64_t gend = min(wk.end, ngroups);
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
    uint64_t glast = gend - 1;
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
    // the end of the launch.  So does a group of a window that lies past the
    // batch (a launch without the claimed tail): its pass runs on the image,
    // the stores' guard drops its items, and the wave arrives at its round's
    // barrier like the others.  The sched_barrier keeps the loads where they
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
    // (even step k: h0/h1 -> issue h3 (k+1, B), h0 (k+2, A)); a and b are the
    // groups of steps k + 1 and k + 2: s + ss and s + 2 ss inside a pass
    auto step_even2 = [&](uint64_t a, uint64_t b) {
        ldh(h3, a, 1);
        const uint32_t u0 = half0(h0);
        ldh(h0, b, 0);
        return part0(u0, h1);
    };
    auto step_odd2 = [&](uint64_t a, uint64_t b) {
        ldh(h1, a, 1);
        const uint32_t u0 = half0(h2);
        ldh(h2, b, 0);
        return part0(u0, h3);
    };
    // the stores of a 4-step pass over the groups first + j sp
    auto store4 = [&](uint32_t vab, uint32_t vc, uint32_t vd, uint64_t first, uint64_t sp) {
        const uint32_t raw = group_reduce32_quad_span(vab, group_pair_level1(vc, vd, lane), lane);
        const uint64_t item = item_of(first + (li & 3u) * (uint32_t)sp);
        if (li < 4 && item < nitems) out[item] = ~raw;
    };
    uint64_t ran = 0;  // steps run (for the probe)
    if (busy) {
        // (<= cg; with a claimed tail the range's last pass is left to the
        // tail loop, whose first chunk it is.  A window's wave runs all its cg
        // steps, those past the batch on the table image.)
        const uint64_t nsteps = (ord != kK1OrderRanges ? cg : gend - grp) - (tail ? 4u : 0u);
        // (the steps in whole passes, the tail loop's one included)
        const uint64_t nwhole = (nsteps + (tail ? 4u : 0u)) & ~3ull;
        ldh(h0, grp, 0);
        ldh(h1, grp, 1);
        ldh(h2, grp + ss, 0);
        // One exit, at the bottom of each loop: a break between the halves would
        // give the loop header a second (un-waited) predecessor, and the waitcnt
        // pass would then drain every prefetched load there.
        uint64_t k = 0;
        for (; k + 4 <= nsteps; k += 4) {
            // the next pass: ps on, or behind the last whole pass the remainder
            // (both grp + 4 in a range)
            const uint64_t nxt = ord == kK1OrderRanges || k + 8 <= nwhole ? grp + ps : wk.rfirst;
            const uint32_t va = step_even2(grp + ss, grp + 2 * ss);
            const uint32_t vb = step_odd2(grp + 2 * ss, grp + 3 * ss);
            const uint32_t vab = group_pair_level1(va, vb, lane);
            const uint32_t vc = step_even2(grp + 3 * ss, nxt);
            const uint32_t vd = step_odd2(nxt, nxt + ss);
            store4(vab, vc, vd, grp, ss);
            grp = nxt;
            // (the three half-steps in flight stay in flight across it)
            if ((k + 4) % kK1RoundSteps == 0 && owed) {
                k1_round_barrier();
                --owed;
            }
            probe.steps(k + 4);
        }
        ran = k;
        for (; k + 2 <= nsteps; k += 2) {
            const uint32_t va = step_even2(grp + ss, grp + 2 * ss);
            const uint32_t vb = step_odd2(grp + 2 * ss, grp + 3 * ss);
            const uint32_t raw = group_reduce32_pair_span(va, vb, lane);
            const uint64_t item = item_of(li == 0 ? grp : grp + ss);
            if (li < 2 && item < nitems) out[item] = ~raw;
            grp += 2 * ss;
        }
        if (nsteps & 1) {
            const uint32_t raw = group_reduce32_single_span(step_even2(grp + ss, grp + 2 * ss), lane);
            const uint64_t item = item_of(grp);
            if (li == 0 && item < nitems) out[item] = ~raw;
        }
    }
    // (with a claimed tail: the arrival of the pass left to the tail loop, one
    // pass early for every wave of the workgroup alike)
    for (; owed; --owed) k1_round_barrier();
    // The claimed tail.  Every range here is full and a multiple of 4 steps, so
    // the loop above left grp at the range's last pass with that pass's first
    // three half-steps in flight: the pass is this loop's first chunk.  Wave
    // slot t claims index i of sub-pool t with one relaxed agent-scope add
    // (lane 0's, a returning vector atomic) at the top of a chunk and runs
    // chunk 16 i + t behind it: the claim comes back while two steps are
    // checksummed, and the chunk's last two steps prefetch the claimed
    // chunk's first half-steps, so the ring of four stays full across chunks.
    // A failed claim (i >= the sub-pool's chunks) prefetches the table image,
    // as a range's end does, and ends the loop: every wave makes exactly one.
    // No barrier in here and nothing waits for another wave.  The pool's last
    // chunk may be cut: its missing groups load the table image and their
    // items lie past nitems, so the stores' guard drops them.
    if (tail) {
        const uint32_t t = wslot;
        const uint64_t mine = k1_tail_pool_chunks(tl.nchunks, t);
        gend = ngroups;
        glast = ngroups - 1;
        // (the head's address through a VGPR the compiler cannot see through:
        // for a wave-uniform address its atomic optimiser rewrites the add as
        // a wave reduction, whose readfirstlane sits right behind the atomic
        // and waits for it with vmcnt(0), draining the ring)
        typedef __attribute__((address_space(1))) uint32_t gu32;
        gu32 *head = (gu32 *)&ctl->head[t].v;
        asm volatile("" : "+v"(head));
        // (sp: the stride of the chunk's steps; the static part's last pass has
        // its order's, a claimed chunk is four neighbouring groups)
        uint64_t cur = grp, nxt, sp = ss;
        do {
            uint32_t i = 0;
            if (lane == 0) i = __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t va = step_even2(cur + sp, cur + 2 * sp);
            const uint32_t vb = step_odd2(cur + 2 * sp, cur + 3 * sp);
            const uint32_t vab = group_pair_level1(va, vb, lane);
            i = __builtin_amdgcn_readfirstlane(i);
            // (ngroups: no chunk; it and ngroups + 1 load the table image)
            nxt = i < mine ? tl.pool0 + ((uint64_t)i * kK1TailPools + t) * kK1TailSteps : ngroups;
            const uint32_t vc = step_even2(cur + 3 * sp, nxt);
            const uint32_t vd = step_odd2(nxt, nxt + 1);
            store4(vab, vc, vd, cur, sp);
            cur = nxt;
            if constexpr (ORD == kK1OrderWindowStep) sp = 1;
            ran += 4;
            probe.steps(ran);
        } while (nxt < ngroups);
        // The launch's end: one more bare barrier for every wave, behind which
        // every claim of the workgroup has returned (each was waited for above).
        // The last workgroup to count itself done then zeroes the counters for
        // the stream's next launch; no claim can follow it.
        k1_round_barrier();
        if (threadIdx.x < 64) {
            uint32_t old = 0;
            if (lane == 0) old = __hip_atomic_fetch_add(&ctl->done.v, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((uint32_t)__builtin_amdgcn_readfirstlane(old) == gridDim.x - 1 && lane <= kK1TailPools)
                __hip_atomic_store(lane < kK1TailPools ? &ctl->head[lane].v : &ctl->done.v, 0u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    probe.exit();
}

// ctl: null for today's static K1, else the counters of this stream's launches
// (launch_k1, shim_launch.h).
template <bool CRCIN, bool NT>
__global__ __launch_bounds__(1024) void k_fixed(const uint8_t *__restrict__ base, uint64_t stride,
                                                uint64_t nitems, const uint4 *__restrict__ img,
                                                const uint32_t *__restrict__ crc_in,
                                                uint32_t *__restrict__ out, K1Ctl *__restrict__ ctl) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    load_tables(smem, img, kLdsImageK1Bytes);
    k_fixed_body<CRCIN, NT>(base, stride, nitems, img, crc_in, out, blockDim.x, ctl, K1NoProbe{});
}

}  // namespace mcrc_dev
