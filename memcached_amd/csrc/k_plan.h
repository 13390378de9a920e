// k_plan.h -- the planned path around the span kernel: k_count (units and
// blocks per span, the item records), the plan's prefix sums, k_expand (the
// unit records, balanced over the groups) and k_final (R to CRC or verdict).
#pragma once

#include "k_spans.h"

namespace mcrc_dev {

// Work units of span [p, p + len): its segments, less a head segment that
// was one block and whose fragment the span's thread takes (none for len 0).
__device__ __forceinline__ uint32_t span_units(const uint8_t *p, uint32_t len) {
    if (len == 0) return 0;
    const uint32_t vlen = len + grid_pad(p, len);
    const uint32_t ns = nseg_of(vlen);
    const SpanHead h = span_head(p, len);
    return ns - (h.drop && h.g1o == vlen - (uint64_t)(ns - 1) * kSegBytes ? 1u : 0u);
}

// 4 KiB blocks of those nu units: 16 per segment, and the head segment's
// niters (make_unit) when it is one of them.
__device__ __forceinline__ uint32_t span_blocks(const uint8_t *p, uint32_t len, uint32_t nu) {
    if (nu == 0) return 0;
    const uint32_t vlen = len + grid_pad(p, len);
    const uint32_t ns = nseg_of(vlen);
    constexpr uint32_t kSegBlocks = kSegBytes / kBlockBytes;
    if (nu < ns) return kSegBlocks * nu;
    const SpanHead h = span_head(p, len);
    const uint32_t po = h.drop ? (uint32_t)h.g1o : 0u;
    const uint32_t eo = vlen - (ns - 1) * kSegBytes - po;
    return (eo + (uint32_t)((uintptr_t)(p + po) & 15u) + kBlockBytes - 1) / kBlockBytes + kSegBlocks * (ns - 1);
}

// Units and blocks per span (packed, units | blocks << 32: one exclusive scan
// places the work units and the balanced plan's group boundaries), and
// the span's item record with its z (the header is parsed once per launch, and
// the foreign bytes of the head piece are read here: for packed images they
// share a line with the header this pass reads anyway; the tail's are
// cleared by the span kernel and not read, round 5).
// Span i's plan entries: one-block flag, unit count, item record, R = 0.
template <int MODE>
__device__ __forceinline__ void count_item(const SpanArgs &a, uint64_t i, const ItemDesc &it, const Tab8 &t8,
                                           uint64_t *nunit, uint4 *irec, uint8_t *fast, bool whole = false,
                                           uint32_t rwhole = 0u) {
    // a span whose unit is one whole block goes to k_blocks (no units)
    const uint8_t *g1;
    bool none;
    const bool one = it.sane && one_block(it.p, it.len, &g1, &none) && !none;
    fast[i] = one;
    const uint32_t nu = one ? 0u : span_units(it.p, it.len);
    nunit[i] = nu | (uint64_t)span_blocks(it.p, it.len, nu) << 32;
    const uint64_t off = (uint64_t)(it.p - a.base);
    uint32_t z = 0;
    const bool carried = carried_image<MODE>(it.sane, it.aux);  // (MODE 3: k_final compares instead of stamping)
    if (it.sane) {
        // (a whole span's R from the wave, whole_chunks: z = R ^ Z of its pieces)
        z = corr_apply(span_corr_arg(it.p, it.len, MODE == 0 ? it.aux : 0u, t8, whole), t8, a.xpow) ^
            (whole ? rwhole : 0u);
        if (MODE == 1 || carried) z ^= mulmodp_dev(~it.aux, a.xpow[grid_pad(it.p, it.len)]);  // W
    }
    irec[i] = make_uint4((uint32_t)off, (uint32_t)(off >> 32) | (it.sane ? 0u : kInsane) | (carried ? kCarried : 0u),
                         it.len, z);
    a.span_acc[i] = 0u;
}

// R = raw of [ph, Ea) (the pieces as they lie, F_t = [E, Ea) cleared as the
// span kernel clears it) for every lane of the wave whose span is whole
// (span_corr's first case: the thread's alone).  A whole
// span's chain used to run in its lane while the lanes without one idled
// (one whole span in seven on the mixed pages: 0.11 of k_count's 0.21 ms);
// now the wave cuts the pieces of all its whole spans into 128-B chunks and
// every lane takes one: r_c = raw of its <= 8 pieces, shifted past the rest of
// its span (M_{Ea - end}, x^(8 n) from the xpow table), XORed into the span's
// slot (LDS, wave-private).  The chunks cover the pieces [ph, ceil16(E)) only
// (the rest of [ph, Ea) is zeros), the piece holding E cleared from E on.
// ph, e and ea are offsets from gb, which must be a 16-byte aligned address:
// ceil16 of such an offset is ceil16 of the address (k_count passes base
// rounded down, not base).  tests/test_count_whole_model.py restates it, with
// the base's residue.
constexpr uint32_t kCountThreads = 256;
// (128-B chunks: half the x^(8n) multiplies of 64-B ones, mixed pages -0.6 %;
// 256-B chunks' longer lane chains were slower: k_count_chunk_size_ab.txt)
constexpr uint32_t kWholePieces = 8, kWholeChunk = 16 * kWholePieces;  // pieces / bytes per chunk
__device__ __forceinline__ uint32_t whole_chunks(gbyte *gb, bool whole, uint64_t ph, uint64_t e, uint64_t ea,
                                                 const Tab8 &t, const uint32_t *xp, uint32_t *slot) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t e16 = (e + 15u) & ~(uint64_t)15u;  // end of the pieces holding bytes of D
    const uint32_t nch = whole ? (uint32_t)((e16 - ph + kWholeChunk - 1u) / kWholeChunk) : 0u;
    uint32_t inc = nch;  // inclusive chunk count over the wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += v;
    }
    const uint32_t total = (uint32_t)__shfl((int)inc, 63, 64), excl = inc - nch;
    slot[lane] = 0u;
    for (uint32_t base = 0; base < total; base += 64u) {
        const uint32_t q = base + lane;
        // owner = the first lane whose inclusive count exceeds q
        uint32_t s = 0;
#pragma unroll
        for (uint32_t step = 32; step; step >>= 1)
            if ((uint32_t)__shfl((int)inc, (int)(s + step - 1u), 64) <= q) s += step;
        const uint32_t c = q - (uint32_t)__shfl((int)excl, (int)s, 64);
        const uint64_t sph = (uint32_t)__shfl((int)(uint32_t)ph, (int)s, 64) |
                             ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(ph >> 32), (int)s, 64) << 32);
        const uint64_t sea = (uint32_t)__shfl((int)(uint32_t)ea, (int)s, 64) |
                             ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(ea >> 32), (int)s, 64) << 32);
        const uint64_t se = (uint32_t)__shfl((int)(uint32_t)e, (int)s, 64) |
                            ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(e >> 32), (int)s, 64) << 32);
        const uint64_t se16 = (se + 15u) & ~(uint64_t)15u;
        const bool act = q < total;
        const uint64_t c0 = sph + (uint64_t)kWholeChunk * c;
        const uint32_t np = act ? (uint32_t)min((se16 - c0) >> 4, (uint64_t)kWholePieces) : 0u;
        Piece pc[kWholePieces];
#pragma unroll
        for (uint32_t k = 0; k < kWholePieces; ++k) pc[k] = k < np ? ld_piece(gb + c0 + 16u * k) : Piece{0, 0};
        // the last piece of the span: bytes from E on cleared (its first 16 - cl kept)
        if (np && c0 + 16u * np == se16) {
            const uint32_t keep = 16u - (uint32_t)(se16 - se);
            const uint64_t mlo = keep >= 8 ? ~0ull : (1ull << (8 * keep)) - 1ull;
            const uint64_t mhi = keep <= 8 ? 0ull : keep >= 16 ? ~0ull : (1ull << (8 * (keep - 8))) - 1ull;
#pragma unroll
            for (uint32_t k = 0; k < kWholePieces; ++k)
                if (k + 1 == np) pc[k] = Piece{pc[k].lo & mlo, pc[k].hi & mhi};
        }
        uint32_t r = 0;
#pragma unroll
        for (uint32_t k = 0; k < kWholePieces; ++k) {
            const uint32_t nx = t.piece(r, pc[k]);
            r = k < np ? nx : r;
        }
        const uint64_t after = act ? sea - (c0 + 16u * np) : 0u;
        r = after ? mulmodp_dev(r, xpow8_dev(xp, after)) : r;
        if (act) atomicXor(&slot[s], r);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    return whole ? slot[lane] : 0u;
}

template <int MODE>
__global__ __launch_bounds__(kCountThreads) void k_count(SpanArgs a, uint64_t *nunit, uint4 *irec, uint8_t *fast) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    __shared__ __attribute__((aligned(16))) uint32_t s8[kTab8Dwords];
    __shared__ uint32_t wslot[kCountThreads / 64][64];
    const uint64_t n = span_count(a);
    // (a K5 fallback list is usually a few hundred spans on a grid sized for
    // the batch: the workgroups past it leave before copying 20 KiB of tables)
    if ((uint64_t)blockIdx.x * blockDim.x >= n) return;
    const Tab8 t8 = load_tab8(s8, a.tab8);
    // whole_chunks rounds its offsets to pieces, and pieces are 16-byte
    // aligned addresses: it gets offsets from gb = base rounded down to a
    // piece boundary (base itself needs no alignment), so that rounding an
    // offset rounds the address.
    const uint64_t ba = (uintptr_t)a.base & 15u;
    gbyte *const gb = (gbyte *)((uintptr_t)a.base - ba);
    uint32_t *const slot = wslot[threadIdx.x >> 6];
    const uint64_t lane = threadIdx.x & 63u;
    // (a wave-uniform loop: every lane takes part in whole_chunks)
    for (uint64_t i0 = blockIdx.x * (uint64_t)blockDim.x + (threadIdx.x - lane); i0 < n;
         i0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = i0 + lane;
        const bool valid = i < n;
        ItemDesc it{a.base, 0u, 0u, false};
        if (valid) it = fetch_item<MODE>(a, i);
        const uint32_t t = grid_pad(it.p, it.len);
        const uint64_t kh = (uintptr_t)it.p & 15u, off = (uint64_t)(it.p - a.base) + ba;  // (from gb)
        const SpanHead h = span_head(it.p, it.len);
        const bool whole = valid && it.sane && it.len != 0 && h.drop && h.g1o == (uint64_t)it.len + t;
        const uint32_t r = whole_chunks(gb, whole, off - kh, off + it.len, off + it.len + t, t8, a.xpow, slot);
        if (valid) count_item<MODE>(a, i, it, t8, nunit, irec, fast, whole, r);
    }
}

// ---------------------------------------------------------------------------
// The plan's prefix sums (round 4: the library's own kernels instead of
// hipcub's scan and select, so that every kernel that runs several
// workgroups per CU carries the VGPR floor, crc32c_device.h).  Per span k_count
// (or the walk) leaves nunit[i] = units | blocks << 32 and fast[i]; tiles of
// kPlanTile spans are reduced (k_plan_tiles), the tile sums scanned by one
// workgroup (k_plan_scan), and k_expand rescans its tile to place every span:
// units and blocks are summed in 64 bits each (no carry between the fields),
// the fast spans' positions give the compacted list k_blocks reads.
// ---------------------------------------------------------------------------
struct PlanSum {
    uint64_t units, blocks;
    uint32_t fast, pad;
};

__device__ __forceinline__ PlanSum plan_of(uint64_t nu, uint8_t f) {
    return {(uint32_t)nu, nu >> 32, (uint32_t)f, 0u};
}
__device__ __forceinline__ PlanSum plan_add(const PlanSum &x, const PlanSum &y) {
    return {x.units + y.units, x.blocks + y.blocks, x.fast + y.fast, 0u};
}

// Exclusive scan of v over a kPlanThreads workgroup; *total = the sum of all.
// Every thread calls it (two barriers; `sh` holds the wave sums).
__device__ __forceinline__ PlanSum block_scan_excl(PlanSum v, PlanSum *sh, PlanSum *total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    PlanSum inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t u = __shfl_up(inc.units, d, 64), b = __shfl_up(inc.blocks, d, 64);
        const uint32_t f = __shfl_up(inc.fast, d, 64);
        if (lane >= d) inc = plan_add(inc, PlanSum{u, b, f, 0u});
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    PlanSum before{0, 0, 0, 0}, all{0, 0, 0, 0};
    for (uint32_t k = 0; k < kPlanThreads / 64; ++k) {
        if (k < w) before = plan_add(before, sh[k]);
        all = plan_add(all, sh[k]);
    }
    __syncthreads();  // (sh is reused by the next call)
    *total = all;
    return plan_add(before, PlanSum{inc.units - v.units, inc.blocks - v.blocks, inc.fast - v.fast, 0u});
}

// Span i's count record (past n: zero).
__device__ __forceinline__ PlanSum plan_at(const uint64_t *nunit, const uint8_t *fast, uint64_t n, uint64_t i) {
    return i < n ? plan_of(nunit[i], fast[i]) : PlanSum{0, 0, 0, 0};
}

// Tile t's sum (thread-contiguous: thread k holds spans t*kPlanTile + kPlanPer k .. + kPlanPer - 1).
__global__ __launch_bounds__(kPlanThreads) void k_plan_tiles(const uint64_t *nunit, const uint8_t *fast, uint64_t n,
                                                            const uint32_t *dn, PlanSum *tile_sum) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    __shared__ PlanSum sh[kPlanThreads / 64];
    if (dn) n = *dn;
    const uint64_t ntiles = (n + kPlanTile - 1) / kPlanTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i0 = t * kPlanTile + (uint64_t)threadIdx.x * kPlanPer;
        PlanSum s{0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < kPlanPer; ++k) s = plan_add(s, plan_at(nunit, fast, n, i0 + k));
        PlanSum tot;
        (void)block_scan_excl(s, sh, &tot);
        if (threadIdx.x == 0) tile_sum[t] = tot;
    }
}

// Exclusive scan of the tile sums of n spans (*dn when given) by one
// workgroup; *total = the grand total (units, blocks and fast spans of the
// whole batch).
__global__ __launch_bounds__(kPlanThreads) void k_plan_scan(const PlanSum *tile_sum, uint64_t n, const uint32_t *dn,
                                                           PlanSum *tile_pre, PlanSum *total) {
    MCRC_VGPR_FLOOR();
    __shared__ PlanSum sh[kPlanThreads / 64];
    if (dn) n = *dn;
    const uint64_t ntiles = (n + kPlanTile - 1) / kPlanTile;
    PlanSum carry{0, 0, 0, 0};
    for (uint64_t t0 = 0; t0 < ntiles; t0 += kPlanThreads) {
        const uint64_t t = t0 + threadIdx.x;
        PlanSum tot;
        const PlanSum ex = block_scan_excl(t < ntiles ? tile_sum[t] : PlanSum{0, 0, 0, 0}, sh, &tot);
        if (t < ntiles) tile_pre[t] = plan_add(carry, ex);
        carry = plan_add(carry, tot);
    }
    if (threadIdx.x == 0) *total = carry;
}

// Exclusive scan of m 32-bit counts by one workgroup (the device page walk:
// the index of each wbuf's first item; a few thousand wbufs per call).
// out[m] = the total.
__global__ __launch_bounds__(1024) void k_scan32(const uint32_t *in, uint64_t m, uint32_t *out) {
    MCRC_VGPR_FLOOR();
    __shared__ uint32_t sh[16];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint64_t i0 = 0; i0 < m; i0 += 1024) {
        const uint64_t i = i0 + threadIdx.x;
        const uint32_t v = i < m ? in[i] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) sh[w] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t k = 0; k < 16; ++k) {
            before += k < w ? sh[k] : 0u;
            all += sh[k];
        }
        __syncthreads();
        if (i < m) out[i] = carry + before + inc - v;
        carry += all;
    }
    if (threadIdx.x == 0) out[m] = carry;
}

// Write the unit records of span i at its units prefix.  Spans whose units would pass
// `cap` (possible only when spans overlap) are listed in `whole` and processed
// as one unit each by a second pass; *nvalid = records written before the
// first such span (zeroed by the caller: none fit).  Spans of more than kExpandInline segments are listed in `big`
// and expanded by k_expand_big, one workgroup per span.
constexpr uint32_t kExpandInline = 32;
// A device-counted list (K5's fallback: a few hundred images whose length
// bits flipped) lands in one or two tiles, so its long spans go to
// k_expand_big sooner: k_expand 0.031 -> 0.012 ms per 300-page verify; at 8
// for every batch config 3 got 2.4 % slower
// (profiles/r04_ablations/k_expand_inline_ab.txt).
constexpr uint32_t kExpandInlineDn = 8;

// First segment of span i that is a unit (1 when the head segment is not).
__device__ __forceinline__ uint32_t first_seg(const uint8_t *p, uint32_t len, uint32_t nunit) {
    return nunit ? nseg_of(len + grid_pad(p, len)) - nunit : 0u;
}

// Balanced plan (starts != nullptr).  T = the blocks of all units, G = the
// span kernel's 32-lane groups: group g's share starts at block g * per,
// per = ceil(T / G).  A unit holding such boundaries is written as pieces cut
// at them (unit_piece), so unit j, first block bs, lands at record j + C(bs),
// C(bs) = the boundaries before bs, and group g's first record is
// starts[g] = j_g + g (j_g: the unit holding block g * per).  A boundary at a
// unit's first block leaves an empty record, the end of group g - 1's list.
// Round robin (starts == nullptr): unit j is record j.
constexpr uint32_t kBalanceMinPer = 2;
struct Balance {
    uint32_t *starts;
    uint64_t per;  // blocks per group
    uint64_t gm;   // groups with blocks: boundaries 1 .. gm - 1
};

// (total: the batch's grand total from k_plan_scan)
__device__ __forceinline__ Balance balance_of(const PlanSum *total, uint64_t n, uint32_t groups, uint32_t *starts) {
    Balance b{starts, 1, 0};
    if (starts && n) {
        // (at least kBalanceMinPer blocks per group.  One per block cut every
        // unit of a small batch into one record per block, serially in its
        // span's thread of k_expand: ~0.3 ms for 50 images of 1-2 MiB before
        // k_expand_big took the long spans of a device-counted list
        // (kExpandInlineDn).  A segment's 16, the floor until round 5, left a
        // small batch on few groups: K5's fallback list of ~1400 blocks per
        // 300 pages ran as 88 groups of 16 serial blocks, k_spans 0.07 ms.)
        const uint64_t t = total->blocks;
        b.per = max((t + groups - 1) / groups, (uint64_t)kBalanceMinPer);
        b.gm = (t + b.per - 1) / b.per;
    }
    return b;
}

__device__ __forceinline__ uint64_t cuts_before(const Balance &b, uint64_t bs) {
    if (!b.starts || bs == 0 || b.gm == 0) return 0;
    return min((bs + b.per - 1) / b.per - 1, b.gm - 1);
}

// Write unit j (record r, first block bs) as its records.
__device__ __forceinline__ void put_unit(UnitRec *units, const Balance &b, uint64_t j, uint64_t bs, const UnitRec &r) {
    if (!b.starts) {
        units[j] = r;
        return;
    }
    uint64_t idx = j + cuts_before(b, bs);
    const uint32_t nb = r.b.z >> 8;
    uint32_t k0 = 0;
    for (uint64_t g = max((bs + b.per - 1) / b.per, (uint64_t)1); g < b.gm && g * b.per < bs + nb; ++g) {
        const uint32_t kb = (uint32_t)(g * b.per - bs);
        units[idx] = unit_piece(r, k0, kb);
        b.starts[g] = (uint32_t)(idx + 1);
        ++idx;
        k0 = kb;
    }
    units[idx] = unit_piece(r, k0, nb);
}

// Per tile (kPlanTile spans, thread-contiguous as k_plan_tiles): the tile's
// prefix from k_plan_scan plus the exclusive scan inside the tile places every
// span's units (p0), first block (b0) and, for a one-block span, its slot in
// the compacted list fastidx (k_blocks).  The units of a wave's spans are
// written by the whole wave (round 5): unit q of the wave's inline units
// goes to lane q mod 64, which finds its span by a search over the lanes'
// inclusive unit counts -- a span of 16 segments used to take 16 serial
// make_unit / put_unit rounds in its lane while the wave's other lanes
// idled.  A span's units after its first are whole segments, so unit j's
// first block is b0 + (j ? nb0 + S (j - 1) : 0), nb0 = the span's blocks
// less S (ns - 1), S = kSegBytes / 4 KiB.  tests/test_span_balance.py
// restates the placement.
__global__ __launch_bounds__(kPlanThreads) void k_expand(const uint8_t *base, const uint64_t *nunit, const uint8_t *fast,
                                                        const PlanSum *tile_pre, const PlanSum *total, const uint4 *irec,
                                                        uint64_t n, const uint32_t *dn, UnitRec *units, uint64_t cap,
                                                        uint32_t *nvalid, UnitRec *whole, uint32_t *nwhole, uint4 *big,
                                                        uint32_t *nbig, uint32_t *fastidx, uint32_t groups,
                                                        uint32_t *starts) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    __shared__ PlanSum sh[kPlanThreads / 64];
    // the wave's spans' unit and block bases, slot 64 k + lane
    __shared__ uint64_t wp0[kPlanThreads / 64][64 * kPlanPer], wb0[kPlanThreads / 64][64 * kPlanPer];
    if (dn) n = *dn;
    const uint64_t ntiles = (n + kPlanTile - 1) / kPlanTile;
    const Balance bal = balance_of(total, n, groups, starts);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t inline_max = dn ? kExpandInlineDn : kExpandInline;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i0 = t * kPlanTile + (uint64_t)threadIdx.x * kPlanPer;
        uint64_t ck[kPlanPer];
        uint8_t fk[kPlanPer];
        PlanSum s{0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < kPlanPer; ++k) {
            ck[k] = i0 + k < n ? nunit[i0 + k] : 0ull;
            fk[k] = i0 + k < n ? fast[i0 + k] : (uint8_t)0;
            s = plan_add(s, plan_of(ck[k], fk[k]));
        }
        PlanSum tot;
        PlanSum pre = plan_add(tile_pre[t], block_scan_excl(s, sh, &tot));
        uint32_t cnt[kPlanPer];  // units this lane's span k leaves to the wave
#pragma unroll
        for (uint32_t k = 0; k < kPlanPer; ++k) {
            const uint64_t i = i0 + k;
            const uint64_t p0 = pre.units, ns = (uint32_t)ck[k], b0 = pre.blocks;
            cnt[k] = 0;
            wp0[w][64 * k + lane] = p0;
            wb0[w][64 * k + lane] = b0;
            if (i < n) {
                if (fk[k]) fastidx[pre.fast] = (uint32_t)i;
                if (p0 + ns <= cap) {
                    if (ns > inline_max) {
                        big[atomicAdd(nbig, 1u)] = make_uint4((uint32_t)i, (uint32_t)p0, (uint32_t)b0, (uint32_t)(b0 >> 32));
                    } else {
                        cnt[k] = (uint32_t)ns;
                    }
                    // the last span whose units fit: the record count
                    if (i + 1 == n || p0 + ns + (uint32_t)nunit[i + 1] > cap)
                        *nvalid = (uint32_t)(p0 + ns + cuts_before(bal, b0 + (ck[k] >> 32)));
                } else {
                    // (one unit with the span's head rule: the same grid, so the same G1)
                    const uint4 r = irec[i];
                    const uint64_t off = rec_off(r);
                    whole[atomicAdd(nwhole, 1u)] = make_unit(base, off, r.z, r.w, !(r.y & kInsane), (uint32_t)i, kWhole);
                }
            }
            pre = plan_add(pre, plan_of(ck[k], fk[k]));
        }
        // the wave's inline units, one per lane and round
        const uint32_t c = cnt[0] + cnt[1];
        static_assert(kPlanPer == 2, "two spans per lane below");
        uint32_t inc = c;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)inc, d, 64);
            if (lane >= d) inc += v;
        }
        const uint32_t T = (uint32_t)__shfl((int)inc, 63, 64), excl = inc - c;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (wp0 / wb0 written above)
        for (uint32_t q0 = 0; q0 < T; q0 += 64u) {
            const uint32_t q = q0 + lane;
            // owner lane: the first whose inclusive count exceeds q
            uint32_t o = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1)
                if ((uint32_t)__shfl((int)inc, (int)(o + step - 1u), 64) <= q) o += step;
            const uint32_t oe = (uint32_t)__shfl((int)excl, (int)o, 64);
            const uint32_t oc0 = (uint32_t)__shfl((int)cnt[0], (int)o, 64);
            if (q < T) {
                const uint32_t r0 = q - oe;
                const uint32_t k = r0 < oc0 ? 0u : 1u;
                const uint32_t j = r0 - (k ? oc0 : 0u);
                const uint64_t i = t * kPlanTile + (uint64_t)((threadIdx.x & ~63u) + o) * kPlanPer + k;
                const uint64_t p0 = wp0[w][64 * k + o], b0 = wb0[w][64 * k + o];
                const uint64_t cki = nunit[i];
                const uint32_t ns = (uint32_t)cki;
                const uint4 r = irec[i];
                const uint64_t off = rec_off(r);
                const uint32_t s0 = first_seg(base + off, r.z, ns);
                const uint64_t nb0 = (cki >> 32) - (uint64_t)(kSegBytes / kBlockBytes) * (ns - 1);
                const uint64_t bs = b0 + (j ? nb0 + (uint64_t)(j - 1) * (kSegBytes / kBlockBytes) : 0u);
                put_unit(units, bal, p0 + j, bs, make_unit(base, off, r.z, r.w, !(r.y & kInsane), (uint32_t)i, s0 + j));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (before the next tile rewrites wp0 / wb0)
    }
}

// big[b] = {span, p0, b0 (lo, hi)} from k_expand.
__global__ void k_expand_big(const uint8_t *base, const uint64_t *nunit, const PlanSum *total, const uint4 *irec,
                             UnitRec *units, const uint4 *big, const uint32_t *nbig, uint64_t n, const uint32_t *dn,
                             uint32_t groups, uint32_t *starts) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    if (dn) n = *dn;
    const Balance bal = balance_of(total, n, groups, starts);
    const uint32_t nb = *nbig;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint4 e = big[b];
        const uint32_t i = e.x;
        const uint64_t p0 = e.y, b0 = e.z | ((uint64_t)e.w << 32);
        const uint32_t ns = (uint32_t)nunit[i];
        const uint4 r = irec[i];
        const uint64_t off = rec_off(r);
        const bool sane = !(r.y & kInsane);
        const uint32_t s0 = first_seg(base + off, r.z, ns);
        // every unit after the first is a whole segment
        const uint32_t nb0 = make_unit(base, off, r.z, r.w, sane, i, s0).b.z >> 8;
        for (uint32_t s = threadIdx.x; s < ns; s += blockDim.x)
            put_unit(units, bal, p0 + s, b0 + (s ? nb0 + (s - 1) * (kSegBytes / kBlockBytes) : 0u),
                     make_unit(base, off, r.z, r.w, sane, i, s0 + s));
    }
}

// Every span's result from its R (one thread per span):
//   planned (UNITS): R = span_acc[i], z from the item record: MODE 1 checks
//   R == W, MODE 0/2 compute ~M_{-t}(R ^ Z), MODE 3 does either by the
//   record's kCarried;
//   one unit per span (MODE 0, no plan): R = out[i], Z computed here.
template <int MODE, bool UNITS>
__global__ void k_final(SpanArgs a, const uint4 *irec) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    __shared__ __attribute__((aligned(16))) uint32_t s8[UNITS ? 1 : kTab8Dwords];
    Tab8 t8{s8};
    if (!UNITS) t8 = load_tab8(s8, a.tab8);
    uint32_t nb = 0;  // bad spans seen by this thread
    const uint64_t n = UNITS ? span_count(a) : a.n;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t *p;
        uint32_t len, R, z = 0;
        bool sane, carried = false;
        if (UNITS) {
            const uint4 r = irec[i];
            carried = MODE == 3 && (r.y & kCarried);
            p = a.base + rec_off(r);
            sane = !(r.y & kInsane);
            len = r.z;
            z = r.w;
            R = a.span_acc[i];
        } else {
            const uint64_t off = a.offsets ? a.offsets[i] : i * a.stride;
            sane = off <= a.base_bytes && a.len <= a.base_bytes - off;  // as decode_unit
            p = a.base + (sane ? off : 0);
            len = a.len;
            const SpanHead h = span_head(p, len);
            // (a span of no bytes or all its thread's is not given to k_spans: out[i] still holds the caller's word)
            R = sane && len != 0 && !(h.drop && h.g1o == len + grid_pad(p, len)) ? a.out[i] : 0u;
            if (sane) z = span_corr(p, len, a.crc_in ? a.crc_in[i] : 0u, t8, a.xpow);
        }
        if (MODE == 1) {
            const bool good = sane && R == z;
            a.ok[i] = good;
            nb += !good;
        } else if (carried) {  // (sane; nothing is written to the image)
            const bool good = R == z;
            if (a.ok) a.ok[i] = good ? kItemKept : 0;
            nb += !good;
        } else {
            const uint32_t t = grid_pad(p, len);
            uint32_t v = R ^ z;
            if (t) v = mulmodp_dev(v, a.xpow[kXpowInv + t]);
            nb += emit<MODE>(a, i, ~v, sane, p);
        }
    }
    count_bad(a.nbad, nb);
}

}  // namespace mcrc_dev
