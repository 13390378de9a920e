// k_blocks.h -- K4: one-block units (K1's loop over gathered blocks).
//
// A span whose unit is exactly one 4 KiB block starting on its grid (its head
// fragment went to its thread: every 4133-B item of configs 2r and 5) needs
// none of the span kernel's unit machinery.  k_blocks runs K1's loop (four
// steps reduced by one tree, no row folds) over those blocks, with each
// group's block address gathered per span instead of base + i * stride,
// and writes R (no initial value, no final XOR): out[i] without a plan,
// span_acc[i] with one.  A span's descriptor is loaded two steps before its
// block: vmcnt counts in issue order, so when the address is needed only the
// newer block loads may still be pending.
#pragma once

#include "k_spans.h"
#include "k_window.h"

namespace mcrc_dev {

struct BlkRegs {
    K1Regs d;       // the block, in K1's lane layout
    uint4 rec;      // descriptor of the block this buffer loads next
    uint32_t rs;    // (planned) its span
    uint32_t sidx;  // (planned) the span of the block two loads later
    uint32_t cur;   // (planned) the span of the block in d
    uint32_t tl;    // the block's span ends tl bytes before the block's end (F_t, mask_tail)
};

template <bool IDENT, bool OFFS>
__global__ __launch_bounds__(1024) void k_blocks(SpanArgs a, const uint4 *__restrict__ img, const uint4 *irec,
                                                 const uint32_t *fastidx, const uint32_t *nfast) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // without a plan block j is span j; with one, span fastidx[j] of the nfast
    // spans k_count found to be one block
    const uint64_t n = IDENT ? a.n : (uint64_t)*nfast;
    const uint64_t waves = blockDim.x >> 6;
    const uint64_t gstep = gridDim.x * waves;
    const uint64_t ngroups = (n + 1) / 2;
    uint64_t grp = __builtin_amdgcn_readfirstlane(blockIdx.x * (uint32_t)waves + (threadIdx.x >> 6));
    if ((uint64_t)blockIdx.x * waves >= ngroups) return;
    load_tables(smem, img, kLdsImageK1Bytes);
    if (grp >= ngroups) return;
    const uint32_t lane = threadIdx.x & 63u, li = lane & 31u, g = lane >> 5;
    const LaneCtx c = make_lane_ctx(li);
    const uint8_t *zero = reinterpret_cast<const uint8_t *>(zero_slot(a));
    auto item_of = [&](uint64_t gi) { return gi * 2 + g; };
    // block index of step gi (past the batch: a repeat of a step of this
    // wave, cache-hot, as in K1's last prefetch; its result is not stored)
    // (32-bit: the shim keeps n below 2^32)
    const uint32_t n32 = (uint32_t)n, ng32 = (uint32_t)ngroups, gstep32 = (uint32_t)gstep;
    auto j_of = [&](uint64_t gi64) -> uint32_t {
        const uint32_t gi = (uint32_t)gi64;
        const uint32_t gu = gi < ng32 ? gi : gi - gstep32 < ng32 ? gi - gstep32 : ng32 - 1;
        const uint32_t j = gu * 2 + g;
        return j < n32 ? j : n32 - 1;
    };
    // descriptor of block j (planned: of its span sj)
    auto rec_of = [&](uint32_t j, uint32_t sj) -> uint4 {
        if (IDENT) {
            // (offsets or stride is a template choice: a load under a branch
            // leaves the waitcnt pass a merged state that drains the prefetch)
            const uint64_t off = OFFS ? a.offsets[j] : j * a.stride;
            return make_uint4((uint32_t)off, (uint32_t)(off >> 32), a.len, 0u);
        }
        return irec[sj];
    };
    // A span here is one whole block and has a unit (one_block), so its block
    // is [Ea - 4096, Ea) whichever case of one_block holds.
    auto block_of = [&](const uint4 &r) -> const uint8_t * {
        const uint64_t off = rec_off(r);
        bool sane = !(r.y & kInsane);
        if (IDENT) sane = off <= a.base_bytes && r.z <= a.base_bytes - off;  // (as decode_unit)
        const uint8_t *e = a.base + off + r.z;
        const uint8_t *blk = e + ((0u - (uint32_t)(uintptr_t)e) & (kGridAlign - 1)) - kBlockBytes;  // (pointer
        return sane ? blk : zero;  // arithmetic: an integer round trip would make these flat loads)
    };
    // t = Ea - E of the block's span (its F_t is the block's last t bytes)
    auto tail_of = [&](const uint4 &r) -> uint32_t {
        return (0u - ((uint32_t)(uintptr_t)a.base + r.x + r.z)) & (kGridAlign - 1);
    };
    // Loads run ahead of their use (vmcnt counts in issue order, so when a
    // value is needed only newer loads may be pending): the span index four
    // steps ahead, the descriptor two, the block one.
    auto ld = [&](BlkRegs &b, uint64_t gi) {
        if (IDENT && !OFFS) {  // (fixed stride: nothing to load ahead)
            const uint4 r = rec_of(j_of(gi), 0u);
            b.tl = tail_of(r);
            b.d.load_at(block_of(r), li * kK1LaneBytes);
        } else {
            const uint8_t *blk = block_of(b.rec);
            b.tl = tail_of(b.rec);
            if (!IDENT) {
                b.cur = b.rs;
                b.rs = b.sidx;
            }
            b.rec = rec_of(j_of(gi + 2 * gstep), b.rs);
            if (!IDENT) b.sidx = fastidx[j_of(gi + 4 * gstep)];
            b.d.load_at(blk, li * kK1LaneBytes);
        }
        // (as K1: the loads stay at the top of the step instead of being sunk
        // into the chains, where the next step would wait on them at once)
        __builtin_amdgcn_sched_barrier(0);
    };
    auto part0 = [&](BlkRegs &b) {
        b.d.d[kK1Pieces - 1] = mask_tail(b.d.d[kK1Pieces - 1], b.tl, li);
        return reduce_level<0>(k1_lane_value(b.d, c), (lane & 1u) == 0u);
    };
    uint32_t *dst = IDENT ? a.out : a.span_acc;
    auto store = [&](uint32_t raw, uint64_t gi, uint32_t span, bool on) {
        const uint64_t item = item_of(gi);
        if (on && gi < ngroups && item < n) dst[IDENT ? item : span] = raw;
    };
    BlkRegs ra, rb;
    if (!IDENT || OFFS) {
        if (!IDENT) {
            ra.rs = fastidx[j_of(grp)];
            rb.rs = fastidx[j_of(grp + gstep)];
            ra.sidx = fastidx[j_of(grp + 2 * gstep)];
            rb.sidx = fastidx[j_of(grp + 3 * gstep)];
        }
        ra.rec = rec_of(j_of(grp), ra.rs);
        rb.rec = rec_of(j_of(grp + gstep), rb.rs);
    }
    const uint64_t nsteps = (ngroups - grp + gstep - 1) / gstep;
    ld(ra, grp);
    uint64_t k = 0;
    for (; k + 4 <= nsteps; k += 4) {
        ld(rb, grp + gstep);
        const uint32_t va = part0(ra), sa = ra.cur;
        ld(ra, grp + 2 * gstep);
        const uint32_t vb = part0(rb), sb = rb.cur;
        const uint32_t vab = group_pair_level1(va, vb, lane);
        ld(rb, grp + 3 * gstep);
        const uint32_t vc = part0(ra), sc = ra.cur;
        ld(ra, grp + 4 * gstep);
        const uint32_t vd = part0(rb), sd = rb.cur;
        const uint32_t raw = group_reduce32_quad_span(vab, group_pair_level1(vc, vd, lane), lane);
        const uint32_t sp = li == 0 ? sa : li == 1 ? sb : li == 2 ? sc : sd;
        store(raw, grp + (li & 3u) * gstep, sp, li < 4);
        grp += 4 * gstep;
    }
    for (; k + 2 <= nsteps; k += 2) {
        ld(rb, grp + gstep);
        const uint32_t va = part0(ra), sa = ra.cur;
        ld(ra, grp + 2 * gstep);
        const uint32_t vb = part0(rb), sb = rb.cur;
        const uint32_t raw = group_reduce32_pair_span(va, vb, lane);
        store(raw, li == 0 ? grp : grp + gstep, li == 0 ? sa : sb, li < 2);
        grp += 2 * gstep;
    }
    if (nsteps & 1) {
        store(group_reduce32_single_span(part0(ra), lane), grp, ra.cur, li == 0);
    }
}

}  // namespace mcrc_dev
