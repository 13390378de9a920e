// k_spans.h -- K2/K3: arbitrary spans, one 32-lane group per work unit (what
// the span kernel computes of a span: k_common.h, "Pieces as they lie").
//
// Work units.  A virtual span longer than kSegBytes is cut into segments of
// kSegBytes anchored at Ea (segment 0, the head, holds the remainder: 17 B to
// kSegBytes + 16 B); every segment is one work unit, so no group owns much
// more than 64 KiB and a batch of
// Zipf-sized items balances over the grid.  Units come from k_count ->
// exclusive scan -> k_expand; a batch whose spans all fit one unit uses unit
// u = span u directly.  Segment units shift their value into place and XOR it
// into the span's accumulator:
//   R(span) = sum_s M_{kSegBytes * (nseg-1-s)}(R(segment s)),
// then k_final turns R into the CRC (or the verdict) of every span.
//
// Unit geometry (the K1 geometry: CH = 32, LPI = 32): a unit [p, e), e
// 16-aligned, is covered by `niters` blocks of 4 KiB anchored at e; block k
// covers [G + 4096k, G + 4096(k+1)), G = e - 4096 * niters, as four 1 KiB rows.
// Lane li owns bytes [32 li, 32 li + 32) of every row (two 16-B pieces) and
// runs one chain per row; rows wholly before p (for every lane of the wave)
// are skipped.  Per block a lane folds
//   acc = M_4096(acc) ^ (((s0 M_1024 ^ s1) M_1024 ^ s2) M_1024 ^ s3),
// and the lane accumulators merge in the K1 lane-group reduction.
//
// Loads are 16-B aligned pieces that overlap [p, E) (so they never leave the
// pages holding the span); a piece wholly outside is read from a zeroed device
// buffer instead, so no load is predicated.
#pragma once

#include "k_common.h"

namespace mcrc_dev {

// Work-unit record written by k_expand (32 B, one dwordx4 pair per unit):
//   a = {offset of the unit's first byte from base (lo, hi), e - p, E - p}
//   b = {z (the span's item record), span index, flags | niters << 8,
//        4 KiB blocks from e to the span's end: (kSegBytes / 4 KiB) (nseg - 1 - segment), more for a piece}
struct alignas(16) UnitRec {
    uint4 a, b;
};

// Decoded descriptor of one work unit (two are live per lane).
struct UnitDesc {
    const uint8_t *p;  // first byte of this unit
    uint32_t eo;       // e - p: e = 16-aligned end of this unit's grid
    uint32_t nf;       // niters << 12 | tail << 4 | flags (tail: bytes of F_t before e, the
                       // span's grid end, when this unit ends there; else 0)
    uint32_t raw;      // this lane's dword li & 7 of the unit's raw record: span index (dword 5)
                       // and segment (dword 7) are gathered from it when the unit ends
    static constexpr uint32_t kValid = 1, kSingle = 2, kHead = 4, kSane = 8;
    static constexpr uint32_t kNitersShift = 12, kTailShift = 4;
    __device__ __forceinline__ uint32_t niters() const { return nf >> kNitersShift; }
    __device__ __forceinline__ uint32_t tail() const { return (nf >> kTailShift) & 127u; }
    __device__ __forceinline__ bool valid() const { return nf & kValid; }
    __device__ __forceinline__ bool single() const { return nf & kSingle; }
    __device__ __forceinline__ bool head() const { return nf & kHead; }
    __device__ __forceinline__ bool sane() const { return nf & kSane; }
};

// Unit (segment `seg` of span [base + off, +len), or the whole span) as a record.
__device__ __forceinline__ UnitRec make_unit(const uint8_t *base, uint64_t off, uint32_t len, uint32_t aux,
                                             bool sane, uint32_t item, uint32_t seg) {
    const uint8_t *p0 = base + off;
    const uint32_t vlen = len + grid_pad(p0, len);
    const uint32_t nseg = seg == kWhole ? 1u : nseg_of(vlen);
    const bool single = nseg == 1, head = single || seg == 0;
    const uint32_t eo0 = vlen - (single ? 0u : (nseg - 1 - seg) * kSegBytes);  // e - p0
    uint32_t po = head ? 0u : eo0 - kSegBytes;                                // p - p0
    if (head) {  // a head fragment taken by the span's thread: the unit starts at G1
        const SpanHead h = span_head(p0, len);
        if (h.drop) po = (uint32_t)h.g1o;
    }
    const uint32_t eo = eo0 - po;
    const uint32_t niters = len ? (eo + (uint32_t)((uintptr_t)(p0 + po) & 15u) + kBlockBytes - 1) / kBlockBytes : 0u;
    const uint64_t o = off + po;
    UnitRec r;
    r.a = make_uint4((uint32_t)o, (uint32_t)(o >> 32), eo, len - po);
    r.b = make_uint4(aux, item,
                     UnitDesc::kValid | (single ? UnitDesc::kSingle : 0u) | (head ? UnitDesc::kHead : 0u) |
                         (sane ? UnitDesc::kSane : 0u) | (niters << 8),
                     single ? 0u : (nseg - 1 - seg) * (kSegBytes / kBlockBytes));
    return r;
}

// Blocks [k0, k1) of unit r (niters nb) as a record of their own: its end
// moves back by nb - k1 blocks (added to its shift), its start (k0 > 0) to
// block k0's grid point, which is 16-B aligned (the grid is anchored at the
// 16-aligned unit end), so the piece's own grid is the unit's.  A piece is
// never stored whole (not single): its value is shifted and XORed into the
// span's accumulator.  k0 == k1: an empty record (flags 0).
__device__ __forceinline__ UnitRec unit_piece(const UnitRec &r, uint32_t k0, uint32_t k1) {
    const uint32_t nb = r.b.z >> 8;
    if (k0 == 0 && k1 == nb) return r;
    UnitRec q{};
    if (k0 == k1) return q;
    const uint32_t delta = k0 ? r.a.z - kBlockBytes * (nb - k0) : 0u;  // block k0's G - p
    const uint64_t o = ((uint64_t)r.a.x | ((uint64_t)r.a.y << 32)) + delta;
    q.a = make_uint4((uint32_t)o, (uint32_t)(o >> 32), r.a.z - kBlockBytes * (nb - k1) - delta, r.a.w - delta);
    q.b = make_uint4(r.b.x, r.b.y, (r.b.z & (UnitDesc::kValid | UnitDesc::kSane)) | ((k1 - k0) << 8),
                     r.b.w + (nb - k1));
    return q;
}

// Raw fetch of unit u.  The record is the same for every lane of a group, so
// lane j of the group holds only its dword j (one VGPR while the loads are in
// flight); decode_unit gathers the dwords when the unit is needed.  Nothing
// here uses the loaded value (a use would make the wave wait for every older
// load, the block prefetch included): units are fetched two ahead and decoded
// when their loads are long done.  One-unit-per-span batches (no plan) fetch
// only the span's offset (lanes 0/1).
template <bool UNITS>
__device__ __forceinline__ uint32_t fetch_unit(const SpanArgs &a, uint64_t u, uint64_t nunits, uint32_t li) {
    const uint32_t j = li & 7u;
    if (u >= nunits) return 0u;  // flags 0: no unit
    if (UNITS) return reinterpret_cast<const uint32_t *>(a.units + u)[j];
    const uint32_t *src = j < 2u && a.offsets ? reinterpret_cast<const uint32_t *>(a.offsets) + 2 * u + j : nullptr;
    return src ? *src : 0u;
}

// Decode unit u's record (raw: its lane-distributed dwords from fetch_unit).
template <bool UNITS>
__device__ __forceinline__ UnitDesc decode_unit(const SpanArgs &a, uint32_t raw, uint64_t u, uint64_t nunits,
                                                uint32_t lane) {
    const uint32_t g = lane & 32u;
    UnitDesc d;
    d.raw = raw;
    if (UNITS) {
        d.p = a.base + ((uint64_t)__shfl(raw, g | 0, 64) | ((uint64_t)__shfl(raw, g | 1, 64) << 32));
        d.eo = __shfl(raw, g | 2, 64);
        // (record dword 6: niters << 8 | flags; dword 3: E - p, past e for
        // every unit but the span's last, whose tail is e - E = t < 128)
        const uint32_t ew = __shfl(raw, g | 3, 64), r6 = __shfl(raw, g | 6, 64);
        const uint32_t tl = d.eo > ew ? d.eo - ew : 0u;
        d.nf = (r6 & 15u) | (tl << UnitDesc::kTailShift) | ((r6 >> 8) << UnitDesc::kNitersShift);
    } else {
        // unit = span u of `len` bytes at `off`: make_unit(kWhole) restated in
        // 32-bit arithmetic (everything but the address depends on p & 15 only;
        // the generic form cost ~200 VALU per switch)
        static_assert(kBlockBytes == 4096, "shifts below");
        const uint64_t off = a.offsets ? (uint64_t)__shfl(raw, g | 0, 64) | ((uint64_t)__shfl(raw, g | 1, 64) << 32)
                                       : u * a.stride;
        const bool sane = off <= a.base_bytes && a.len <= a.base_bytes - off;  // else: read nothing
        const uint32_t len = sane ? a.len : 0u;
        const uint32_t plo = (uint32_t)(uintptr_t)a.base + (uint32_t)off, kh = plo & 15u;
        const uint32_t vlen = len + ((0u - plo - len) & (kGridAlign - 1));  // grid_pad
        const uint32_t x = vlen + kh;  // Ea - ph
        const uint32_t g1o = x - kBlockBytes * ((x - 1) >> 12) - kh;  // span_head
        const uint32_t po = frag_drop(len, g1o, vlen) ? g1o : 0u;
        const uint32_t eo = vlen - po;
        const uint32_t niters = len ? (eo + ((kh + po) & 15u) + kBlockBytes - 1) >> 12 : 0u;
        d.p = a.base + (sane ? off : 0) + po;
        d.eo = eo;
        d.nf = u < nunits ? UnitDesc::kValid | UnitDesc::kSingle | ((vlen - len) << UnitDesc::kTailShift) |
                                (niters << UnitDesc::kNitersShift)
                          : 0u;  // flags 0: no unit
    }
    return d;
}

// A 4 KiB block of a unit in K1's lane layout (round 5): lane li holds the
// 16-B pieces at G + 512 k + 16 li, k = 0..7, so each load instruction reads
// 512 contiguous bytes per group, non-temporal (k_common.h, "K1's lane
// layout").
// (non-temporal: the planned path's blocks are whole lines since round 5,
// kGridAlign; config 3 -1.5 to -2 %, mixed pages -1.3 % against the row
// layout, profiles/r05_ablations/spans_line_grid_ab.txt)
struct BlockWin {
    uint4 v[kK1Pieces];
};

// Issue the loads of block k of unit d for lane li.
__device__ __forceinline__ void load_block(BlockWin &w, const UnitDesc &d, uint32_t k, uint32_t li,
                                           const uint4 *zero) {
    // Offsets relative to the unit's first byte p: block start G - p = grel;
    // lane li's piece k is [grel + 512 k + 16 li, +16).  A piece that ends at
    // or before ph = floor16(p) reads the zero line (only head blocks have
    // such pieces); every other piece overlaps [ph, e), so no load leaves the
    // pages of the span.
    const int32_t grel = (int32_t)d.eo - (int32_t)(kBlockBytes * (d.niters() - k));
    const int32_t lrel = grel + (int32_t)(kK1LaneBytes * li);
    const uint8_t *q0 = d.p + lrel;
    const uint8_t *zl = reinterpret_cast<const uint8_t *>(zero);
    // piece-0 end - ph; a unit without blocks (no bytes, or no unit) reads
    // nothing but zeros
    const int32_t e0 = d.niters() ? lrel + 16 + (int32_t)((uintptr_t)d.p & 15u) : -(int32_t)kBlockBytes - 16;
#pragma unroll
    for (int j = 0; j < (int)kK1Pieces; ++j) {
        const uint8_t *q = e0 + j * (int32_t)kK1Piece > 0 ? q0 + j * kK1Piece : zl;
        w.v[j] = ld16_nt(q);
    }
}

// F_t cleared: the span's grid ends at Ea = E + t (t < 128), so F_t lies in
// the last line of its last block, piece 7 of lanes 24..31 (lane li's piece
// 7 is the line's bytes [16 (li - 24), +16)); the bytes of that piece from E
// on, min(max(t - 16 (31 - li), 0), 16) of them, are cleared.
__device__ __forceinline__ uint4 mask_tail(uint4 v, uint32_t t, uint32_t li) {
    const int32_t cl = min(max((int32_t)t - 16 * (31 - (int32_t)li), 0), 16);  // bytes cleared
    const int32_t keep = 16 - cl;
    uint32_t m[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int32_t kb = min(max(keep - 4 * i, 0), 4);
        m[i] = kb >= 4 ? ~0u : (1u << (8 * kb)) - 1u;
    }
    return make_uint4(v.x & m[0], v.y & m[1], v.z & m[2], v.w & m[3]);
}

// acc' = M_4096(acc) ^ (the block's lane value) = M_2048(M_2048(acc) ^ u_A) ^ u_B
// (u_A / u_B: the first / second half's chains, k1_lane_value; M_2048 = the
// chunk-16 image's tables 16..19).  NS: rows (piece pairs) 0..NS-1 lie wholly
// before p for every lane of the wave (their chains are of zeros and are
// skipped); fold: some group of the wave is past its unit's first block
// (wave-uniform; else every acc is 0 and is not folded).
// The chains of one half's pieces v[J0..3] (v[j] for j < J0 are zeros and
// are skipped), each ended by its shifted last step: the half's value.  (One
// half at a time: eight live chains beside the prefetched block pushed the
// span kernel past 128 VGPRs into scratch.)
template <int J0>
__device__ __forceinline__ uint32_t half_value(const uint4 *v, const LaneCtx &c) {
    constexpr uint32_t kShift[3] = {kAuxShift0, kAuxShift1, kAuxShift2};
    uint32_t x[4];
#pragma unroll
    for (int j = J0; j < 4; ++j) x[j] = v[j].x;
#pragma unroll
    for (int i = 1; i < 4; ++i)
#pragma unroll
        for (int j = J0; j < 4; ++j) x[j] = step4_next(x[j], dw4(v[j], i), c);
    uint32_t u = 0;
#pragma unroll
    for (int j = J0; j < 4; ++j) u ^= j < 3 ? step4_last_shifted(x[j], kShift[j]) : step4_next(x[j], 0u, c);
    return u;
}

template <int NS>
__device__ __forceinline__ uint32_t block_fold(uint32_t acc, bool fold, const BlockWin &w, const LaneCtx &c) {
    const uint32_t ub = half_value<NS == 3 ? 2 : 0>(w.v + 4, c);
    if (NS >= 2 && !fold) return ub;
    uint32_t h = fold ? apply_op<4>(kAuxSpanFold, acc) : 0u;
    if (NS < 2) h ^= half_value<2 * (NS & 1)>(w.v, c);
    return apply_op<4>(kAuxSpanFold, h) ^ ub;
}

// v * y mod P spread over a 32-lane group: lane i adds bit i of v (the x^i
// coefficient) times xi = x^i * y (this lane's element of a row of the segpow
// table), and the lanes XOR-reduce into lane 0.  v is read from lane 0 of the
// group.
__device__ __forceinline__ uint32_t mul_row_group(uint32_t v0, uint32_t xi, uint32_t li) {
    const uint32_t v = __shfl(v0, 0, 32);
    uint32_t term = (v << li) & 0x80000000u ? xi : 0u;
    term ^= lane_down<0>(term);
    term ^= lane_down<1>(term);
    term ^= lane_down<2>(term);
    term ^= lane_down<3>(term);
    term ^= lane_down<4>(term);
    return term;
}

// The span kernel: R = raw([ph, e)) of every work unit, pieces as they lie.
// A unit that is a whole span stores R (span_acc[span], or out[span] without
// a plan); a segment unit XORs M_{64Ki * (nseg-1-s)}(R) into span_acc[span].
// k_final then turns R into the CRC or the verdict.
template <bool UNITS>
__global__ __launch_bounds__(kSpanBlock) void k_spans(SpanArgs a, const uint4 *__restrict__ img) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint64_t nunits = UNITS ? (uint64_t)*a.nunits : a.n;
    // Balanced plan (k_expand): group g takes the records [starts[g],
    // starts[g + 1]), an equal share of the batch's blocks; else group g takes
    // units g, g + G, g + 2G, ...
    const bool bal = UNITS && a.starts;
    const uint32_t g0 = blockIdx.x * (blockDim.x >> 5);
    // a workgroup without a unit leaves before loading 160 KiB of tables (the
    // overlap pass is usually empty, and small plans do not fill the grid)
    if (bal ? (g0 && a.starts[g0] >= nunits) : (uint64_t)g0 >= nunits) return;
    load_tables(smem, img, kLdsImageK1Bytes);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t li = lane & 31u;
    const LaneCtx c = make_lane_ctx(li);
    const uint64_t ngroups_total = (uint64_t)gridDim.x * (blockDim.x >> 5);
    const uint32_t g = g0 + ((threadIdx.x >> 6) << 1) + (lane >> 5);
    // Rounds (round 5): the balanced plan cuts the batch's blocks into
    // rounds x G equal shares in block order and group g takes shares g,
    // G + g, 2G + g, ..., so the groups stream through one round's range of
    // the batch (about 8 GiB: host_route.h plan_rounds) at a time instead
    // of each through its own 1/G of all of it.  Each round restarts the
    // group's pipeline.
    const uint32_t nrounds = bal ? a.rounds : 1u;
    uint64_t u = g;
    uint64_t ub = nunits;  // the group's records (of this round) end here
    auto share = [&](uint32_t rd) {
        const uint64_t v = (uint64_t)rd * ngroups_total + g;
        u = v ? min(a.starts[v], (uint32_t)nunits) : 0u;
        ub = min(a.starts[v + 1], (uint32_t)nunits);
    };
    if (bal) share(0);
    const uint64_t ustep = bal ? 1u : ngroups_total;

    UnitDesc cur = decode_unit<UNITS>(a, fetch_unit<UNITS>(a, u, ub, li), u, nunits, lane);
    // Ring of the next four units' raw records, lane-distributed: lanes
    // 8s..8s+7 of a group hold slot s.  The unit after cur is in slot sl; a
    // switch decodes it and refills the slot with the unit four further on.
    // Nothing is copied out of the ring and no load is used right after it is
    // issued (vmcnt counts in issue order: either would make the wave wait
    // for the block prefetch too).
    uint32_t ring = fetch_unit<UNITS>(a, u + (1 + (li >> 3)) * ustep, ub, li);
    const uint32_t *const segpow_rows = a.segpow;
    uint32_t sl = 0;
    uint32_t k = 0;    // block index inside cur
    uint32_t acc = 0;  // lane accumulator over the blocks of cur
    BlockWin w0, w1;
    const uint4 *zero = zero_slot(a);
    load_block(w0, cur, 0, li, zero);

    // Process the block held in `w` (block k of cur) after issuing the loads of
    // the group's next block into `wn`.
    auto step = [&](BlockWin &w, BlockWin &wn) {
        const bool last = k + 1 >= cur.niters();
        // next block: block k + 1 of cur, or block 0 of the unit in ring slot sl
        UnitDesc nd;
        if (__any(last)) {
            const uint32_t g = lane & 32u, sb = sl << 3;
            const uint32_t rw = __shfl(ring, g | sb | (li & 7u), 64);  // slot sl, dword li & 7
            nd = decode_unit<UNITS>(a, rw, u + ustep, nunits, lane);
        }
        if (last && (li >> 3) == sl) ring = fetch_unit<UNITS>(a, u + 5 * ustep, ub, li);
        // a segment unit's shift row, loaded after the (masked) ring refill and
        // before the block prefetch: the multiply below then waits for exactly
        // the block's loads issued after it, vmcnt(8), not for everything
        // (under a wave-uniform branch: loads under divergent branches leave
        // the waitcnt pass a merged state that drains the prefetch)
        uint32_t segk = 0, fx1 = 0;
        if (UNITS) {
            segk = __shfl(cur.raw, (lane & 32u) | 7u, 64);
            if (__builtin_amdgcn_readfirstlane(__any(last && !cur.single())))
                fx1 = segpow_rows[32 * (segk & (kSegpowLo - 1)) + li];
            __builtin_amdgcn_sched_barrier(0);  // (issued before the block prefetch, not sunk after it)
        }
        {
            UnitDesc t = cur;
            t.p = last ? nd.p : cur.p;
            t.eo = last ? nd.eo : cur.eo;
            t.nf = last ? nd.nf : cur.nf;
            load_block(wn, t, last ? 0u : k + 1, li, zero);
        }
        // Every path consumes the whole block (a path that skips rows, or a
        // group without a unit, would otherwise leave the block's loads
        // pending in the waitcnt pass's view, and the next write to those
        // registers became an s_waitcnt vmcnt(0) that drained the prefetch).
#pragma unroll
        for (int j = 0; j < (int)kK1Pieces; ++j)
            asm volatile("" ::"v"(w.v[j].x), "v"(w.v[j].y), "v"(w.v[j].z), "v"(w.v[j].w));
        if (cur.niters()) {
            if (__any(last && cur.tail())) w.v[kK1Pieces - 1] = mask_tail(w.v[kK1Pieces - 1], last ? cur.tail() : 0u, li);
            const int32_t grel = (int32_t)cur.eo - (int32_t)(kBlockBytes * (cur.niters() - k));  // G - p
            // rows wholly before p for every lane of the wave are skipped
            // (a group without a unit has niters == 0 and votes to skip)
            const uint32_t nskip = __all(grel + 3 * (int32_t)kRowBytes <= 0)   ? 3u
                                   : __all(grel + 2 * (int32_t)kRowBytes <= 0) ? 2u
                                   : __all(grel + (int32_t)kRowBytes <= 0)     ? 1u
                                                                               : 0u;
            // (the fold of a unit's first block is of acc = 0: skipped when no
            // group of the wave is past its first block, e.g. one-block units)
            const bool fold = __builtin_amdgcn_readfirstlane(__any(k != 0));
            switch (nskip) {
                case 0: acc = block_fold<0>(acc, fold, w, c); break;
                case 1: acc = block_fold<1>(acc, fold, w, c); break;
                case 2: acc = block_fold<2>(acc, fold, w, c); break;
                default: acc = block_fold<3>(acc, fold, w, c); break;
            }
        }
        if (last) {
            if (cur.valid()) {
                const uint32_t raw = group_reduce32_span(acc, lane);
                if (!UNITS) {
                    if (li == 0) a.out[u] = raw;
                } else {
                    const uint32_t item = __shfl(cur.raw, (lane & 32u) | 5u, 64);
                    if (cur.single()) {
                        if (li == 0) a.span_acc[item] = raw;
                    } else {
                        // a segment or piece ending segk blocks before the span's end:
                        // R(span) gets M_{4096 segk}(R) (the second factor, for units
                        // 16 MiB or more before the end only, is loaded here:
                        // one register fewer across the step, a drain only at such segment ends)
                        uint32_t v = mul_row_group(raw, fx1, li);
                        if (__any(segk >= kSegpowLo))
                            v = mul_row_group(v, segpow_rows[32 * (kSegpowLo + segk / kSegpowLo) + li], li);
                        if (li == 0) atomicXor(a.span_acc + item, v);
                    }
                }
            }
            acc = 0;
            k = 0;
            u += ustep;
            cur = nd;
            sl = (sl + 1u) & 3u;
        } else {
            ++k;
        }
    };

    for (uint32_t rd = 0;;) {
        // nothing issued before the loop stays pending into it (the waitcnt
        // pass would otherwise wait for it, vmcnt(0), at the top of every
        // iteration)
        __builtin_amdgcn_s_waitcnt(0);
        // One, wave-uniform exit at the bottom (a group that has finished
        // runs empty steps until the other has): a divergent or mid-loop exit
        // gives the loop header an un-waited predecessor, and the waitcnt
        // pass then drains the prefetch there (vmcnt(0)) on every iteration.
        for (;;) {
            step(w0, w1);
            step(w1, w0);
            if (!__builtin_amdgcn_readfirstlane(__any(cur.valid()))) break;
        }
        if (++rd >= nrounds) break;
        // (a round whose first share is empty is followed by empty ones: a
        // small plan -- K5's fallback list -- fills round 0 or less)
        if (a.starts[(uint64_t)rd * ngroups_total] >= (uint32_t)nunits) break;
        // the next round's share: a fresh pipeline (the ring and the block
        // prefetch of the finished share hold nothing of it)
        share(rd);
        cur = decode_unit<UNITS>(a, fetch_unit<UNITS>(a, u, ub, li), u, nunits, lane);
        ring = fetch_unit<UNITS>(a, u + (1 + (li >> 3)) * ustep, ub, li);
        sl = 0;
        k = 0;
        acc = 0;
        load_block(w0, cur, 0, li, zero);
    }
}

}  // namespace mcrc_dev
