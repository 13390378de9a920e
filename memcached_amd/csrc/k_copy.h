// k_copy.h -- crc32c_copy_items: item images copied and verified in one pass.
#pragma once

#include "copy_edges.h"
#include "k_small.h"

namespace mcrc_dev {

// The destination side of a copy (the source side is SpanArgs, as for a
// verify: base, base_bytes, offsets, region, cfl, ok, nbad, host_nbad, done).
struct CopyArgs {
    uint8_t *dst;                 // image i goes to dst + dst_offsets[i]
    uint64_t dst_bytes;
    const uint64_t *dst_offsets;
    uint32_t *nrange;             // sane images that do not fit dst (atomic; the last workgroup
                                  // moves it to host_nbad[1] and zeroes it)
};

// ok[] values of a copy (CRC32C_ITEM_COPIED / _DAMAGED, crc32c_batch.h).
constexpr uint8_t kItemCopied = 1, kItemDamaged = 3;

// Destination bytes, in the global address space (a generic pointer's stores
// are flat ones, which also count in lgkmcnt: k_common.h, gbyte), written at
// any alignment: global memory takes unaligned stores on gfx950 (emit,
// k_common.h, relies on that for a dword).
typedef __attribute__((address_space(1))) uint8_t gwbyte;
typedef u32x4 u32x4_u __attribute__((aligned(1)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_u __attribute__((aligned(1)));
typedef uint32_t u32_u __attribute__((aligned(1)));
typedef uint16_t u16_u __attribute__((aligned(1)));

__device__ __forceinline__ void st16(gwbyte *d, const uint4 &v) {
    u32x4 x;
    x.x = v.x, x.y = v.y, x.z = v.z, x.w = v.w;
    *(__attribute__((address_space(1))) u32x4_u *)d = x;
}

// Bytes [from, from + n) of piece v to d (n = 1..16, from + n <= 16): the
// stores of mcrc::edge_widths.  The piece is moved down by `from` bytes with
// v_alignbyte_b32 (no 64-bit shift: parse_hdr, k_common.h).
__device__ __forceinline__ void store_edge(gwbyte *d, const uint4 &v, uint32_t from, uint32_t n) {
    if (n >= 16u) {
        st16(d, v);
        return;
    }
    const uint32_t s[8] = {v.x, v.y, v.z, v.w, 0u, 0u, 0u, 0u};
    const uint32_t qi = from >> 2, b = from & 3u;
    uint32_t w[5], o[4];
#pragma unroll
    for (uint32_t m = 0; m < 5; ++m) w[m] = qi == 0 ? s[m] : qi == 1 ? s[m + 1] : qi == 2 ? s[m + 2] : s[m + 3];
#pragma unroll
    for (uint32_t m = 0; m < 4; ++m) o[m] = __builtin_amdgcn_alignbyte(w[m + 1], w[m], b);
    // edge_widths(n): the set bits of n from 8 down, each store at a multiple
    // of its width from d
    uint32_t pos = 0;
    if (n & 8u) {
        u32x2_u y;
        y.x = o[0], y.y = o[1];
        *(__attribute__((address_space(1))) u32x2_u *)d = y;
        pos = 8;
    }
    if (n & 4u) {
        *(__attribute__((address_space(1))) u32_u *)(d + pos) = pos ? o[2] : o[0];
        pos += 4;
    }
    const uint32_t q = pos >> 2;
    uint32_t x = q == 0 ? o[0] : q == 1 ? o[1] : q == 2 ? o[2] : o[3];  // (pos is a multiple of 4 here)
    if (n & 2u) {
        *(__attribute__((address_space(1))) u16_u *)(d + pos) = (uint16_t)x;
        x >>= 16;
        pos += 2;
    }
    if (n & 1u) d[pos] = (uint8_t)x;
}

// k_copy: one 32-lane group per image, the groups striding over the list
// (group g takes images g, g + G, ...: one launch serves 1 image or 10
// million).  Per image it is k_small's verify -- the whole span [ph, Ea) in
// 4 KiB blocks anchored at Ea, the next block loaded before the current one is
// folded, R compared with W = Z ^ M_t(~stored CRC) -- and every block's pieces
// are also stored at dst + (address - image start), at the destination's own
// byte alignment.  Of the pieces that hold a byte of the image
// (mcrc::copy_plan: piece k = image bytes [16 k - sa, +16)) the blocks hold
// 2 .. npieces - 1 and store the whole ones, one predicated 16-B store per
// piece.  The pieces that straddle an image edge are stored by lane 0 after
// the blocks, narrower (store_edge): the last piece when the image ends inside
// it, from the load that Z's raw(F_t) needs anyway, and piece 0 when sa != 0
// (it reads up to 15 bytes in front of the image, inside the 16-B granule of
// the image's first byte); with piece 0 goes piece 1, the rest of the 32 - sa
// bytes in front of the span's first piece.
// (Realigning the pieces in registers so that every 16-B store is aligned was
// not built: destinations placed at their source's alignment measure the same
// as packed ones, and with the stores compiled out the kernel keeps 80 % of
// its time -- DESIGN.md section 3.7, profiles/copy_items_ab.jsonl.)
// An image that is not sane, or does not fit dst, is neither read nor
// written; a damaged one is written whole (its verdict is known only after
// its last byte).  A long image stays on its one group.
__global__ __launch_bounds__(1024) void k_copy(SpanArgs a, CopyArgs ca, const uint4 *__restrict__ img) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    load_tables(smem, img, kLdsImageK1Bytes);
    const uint32_t lane = threadIdx.x & 63u, li = lane & 31u;
    const LaneCtx c = make_lane_ctx(li);
    const uint32_t gpb = blockDim.x >> 5;
    const uint64_t G = (uint64_t)gridDim.x * gpb;
    const uint4 *zero = zero_slot(a);
    uint32_t nb = 0, nr = 0;  // (lane 0 of a group: its bad images, its images that did not fit)
    for (uint64_t i = (uint64_t)blockIdx.x * gpb + (threadIdx.x >> 5);
         __builtin_amdgcn_readfirstlane(__any(i < a.n)); i += G) {
        const bool valid = i < a.n;
        ItemDesc it{a.base, 0u, 0u, false};
        uint64_t doff = 0;
        if (valid) {
            it = fetch_item<1>(a, i);
            doff = ca.dst_offsets[i];
        }
        const uint64_t nt = (uint64_t)it.len + 32u;
        const bool fits = doff <= ca.dst_bytes && nt <= ca.dst_bytes - doff;
        const bool go = it.sane && fits;
        const uint32_t len = go ? it.len : 0u;
        const uint32_t sa = (uint32_t)((uintptr_t)it.p & 15u);  // (image start = p - 32)
        const mcrc::CopyPlan plan = mcrc::copy_plan(sa, 0u, nt);
        gwbyte *const dimg = (gwbyte *)ca.dst + (go ? doff : 0u);
        const uint32_t hd = 32u - sa, whole_max = (uint32_t)nt - 16u - hd;  // (nt >= 50 when anything is stored)
        const uint32_t t = tail_pad(it.p, len), eo = len + t;
        const uint32_t niters = len ? (eo + sa + kBlockBytes - 1) / kBlockBytes : 0u;
        const uint32_t nmax = __builtin_amdgcn_readfirstlane(max(niters, (uint32_t)__shfl_xor(niters, 32, 64)));
        uint32_t acc = 0;
        // block k + 1 is loaded before block k is stored and reduced (two register sets)
        auto issue = [&](BlockWin &w, uint32_t k) {
            UnitDesc d;
            d.p = it.p;
            d.eo = eo;
            d.nf = k < niters ? (niters << UnitDesc::kNitersShift) | UnitDesc::kValid : 0u;
            d.raw = 0;
            load_block(w, d, k, li, zero);
        };
        auto reduce = [&](const BlockWin &w, uint32_t k) {
            if (k < niters) {
                // lane li's piece j is image bytes [r, r + 16), r = x + hd: a whole
                // store when hd <= r <= nt - 16 (hd = 32 - sa, where piece 2 starts;
                // pieces in front of it were read from the zero line), one compare
                const uint32_t x0 = eo + sa - kBlockBytes * (niters - k) + kK1LaneBytes * li;
                gwbyte *const d0 = dimg + hd + (int32_t)x0;
#pragma unroll
                for (int j = 0; j < (int)kK1Pieces; ++j) {
                    const uint32_t x = x0 + j * kK1Piece;
                    if (x <= whole_max) st16(d0 + j * kK1Piece, w.v[j]);
                }
            }
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
        if (valid) {
            // W on k_small's 16-B grid (k_small.h): Z = M_{len+t}(~0 ^ raw(F_h)) ^ raw(F_t)
            uint32_t z = 0;
            if (len) {
                uint32_t y = ~0u;
                if (sa) y ^= raw16_img(shl_bytes(ld_piece(it.p - sa), 16 - sa), c);
                z = mulmodp_dev(y, xpow8_dev(a.xpow, (uint64_t)len + t));
                const uint8_t *const qt = it.p + len + t - 16;  // the last piece
                if (t) z ^= raw16_img(clear_below(ld_piece(qt), 16 - t), c);
                if (li == 0) {
                    // the pieces that straddle the image's edges, and piece 1
                    const uint8_t *const q0 = it.p - 32 - sa;
                    const uint4 h0 = ld16(q0), h1 = ld16(q0 + 16);
                    store_edge(dimg, h0, sa, plan.head);
                    st16(dimg + plan.head, h1);
                    if (t) store_edge(dimg + (nt - plan.tail), ld16(qt), 0u, plan.tail);
                }
            }
            const bool good = go && R == (z ^ mulmodp_dev(~it.aux, a.xpow[t]));
            if (li == 0) {
                a.ok[i] = !go ? 0 : good ? kItemCopied : kItemDamaged;
                nb += !good;
                nr += it.sane && !fits;
            }
        }
    }
    // one atomic per wave and counter (all 160 KiB of LDS hold the tables)
    wave_sum(nb);
    wave_sum(nr);
    if (lane == 0 && (nb | nr)) {
        if (nb) atomicAdd(a.nbad, (unsigned long long)nb);
        if (nr) atomicAdd(ca.nrange, nr);
        __threadfence();  // (performed before this workgroup is counted done: k_small.h)
    }
    // the last workgroup hands both counts to the host and leaves the counters
    // at zero for the next call, as k_small's does
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(a.done, 1u) == gridDim.x - 1) {
            __threadfence();
            a.host_nbad[0] = atomicExch(a.nbad, 0ull);
            a.host_nbad[1] = atomicExch(ca.nrange, 0u);
            atomicExch(a.done, 0u);
            __threadfence_system();
        }
    }
}

}  // namespace mcrc_dev
