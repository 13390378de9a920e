// k_lines.h -- K5: item images or equal spans whose span is one 4 KiB window
// of whole lines after a short head (k_lines, line-anchored since round 4),
// with k_fix (a stamp's last step) and k_census (K5 or the planned path).
//
// Images that are sane but not of K5's shape go to a fallback list that the
// planned path takes afterwards; malformed images are marked bad by K5.
//
// Round 3's K5 (k_items, removed in round 5; git show 7745007) read each
// image's header and head fragment at the start of an epoch and the image's
// 16-B-anchored block up to 32 steps later, by when the
// lines they share (the block's first line, the previous block's last line,
// which holds this image's header) have left L2: config 5 fetched 1.08x its
// span bytes, config 2r 1.065x (profiles/r04_ablations).  Here no line is
// read by both a block and a per-lane prep:
//   - the block of span D = [p, E) is the window [A, A + 4096), A =
//     ceil128(p + 4): the whole lines [A, B) of D, B = floor128(E), and zeros
//     past B (31 or 32 lines: the fused shape; lanes 28-31 of row 3 read the
//     zero line for a 31-line window);
//   - the epoch lane of the image takes its head [p, A) (4..131 bytes, ~c
//     injected at p: r_h = register from ~c over [p, A)) and its tail
//     [B, Et), Et = ceil16(E), bytes from E on cleared (r_t);
//   - a wave's epoch is a run of 2 nsr CONSECUTIVE images (lane L prepares
//     image L of the run, step s checksums images 2s and 2s + 1), so one
//     image's tail and the next image's head and header -- the same one or
//     two lines -- are read by neighbouring lanes of one instruction;
//   - the group's R = raw of the window goes back to the image's epoch lane,
//     which at the end of the run forms
//       V = M_{Et-A}(r_h) ^ M_{Et-A-4096}(R) ^ r_t = M_pad(f),
//     f the register after D from ~c, pad = Et - E: crc32c(c, D) =
//     ~M_{-pad}(V); a verify is good iff V == M_pad(~stored).  Round 6: the
//     lane forms W = M_128(V) = M_d(M_4096(r_h) ^ R) ^ M_128(r_t), d = Et - A
//     - 3968 in [0, 272), with the table operators (M_2048 twice, the tree
//     levels M_16..M_128 by the bits of d, zeros_lds below 16) instead of two
//     bitwise multiplies by x^(8 (Et - A)) and x^(8 (Et - A - 4096)) (the
//     second negative for a 31-line window with a short tail, hence the
//     M_128): a verify is good iff W == M_128(M_pad(~stored)), the CRC is
//     ~M_{-pad-128}(W).
// tests/test_items_lines_model.py restates it on the CPU.
#pragma once

#include "k_window.h"

namespace mcrc_dev {

constexpr uint32_t kHeadPieces = 10;  // 16-B pieces of [floor16(p), A): A - p <= 131
constexpr uint32_t kTailPieces = 9;   // of [B, Et): Et - B < 128 + 16
constexpr uint32_t kSt31 = 0x80u;     // the window holds 31 lines (row 3, lanes 28-31: zeros)
constexpr uint32_t kStFused = 0x10u, kStSane = 0x20u, kStValid = 0x40u;


struct ItemsOut {
    uint32_t *fb;   // items for the planned path (sane, not one block)
    uint32_t *nfb;  // their count
    const uint32_t *route;  // k_census's verdict (nullptr: take the batch); 0: every image to the planned path
    uint2 *rt;      // MODE 2/3: per item {M_t(f), t | kRtFused}, {0, 0} if not fused or (MODE 3)
                    // a carried image, which k_lines itself verified (for k_fix)
    uint32_t xm128;      // k_lines: x^(-8 * 128) (MODE 0: the CRC from M_128(V))
    uint32_t nsr;        // k_lines: steps per run (a wave's run is 2 nsr consecutive images)
};
constexpr uint32_t kRtFused = 0x80000000u;

// The dword at A of the head fragment: bytes below p cleared (pa = p - A)
// and the four bytes of inj (~c for an initial CRC c: a register seeded with
// ~c, crc32c.c:166) XORed into the bytes of [p, p + 4) it holds.
__device__ __forceinline__ uint32_t head_dword(uint32_t v, int32_t pa, uint32_t inj) {
    if (pa >= 4) return 0u;
    if (pa >= 0) return (v & (~0u << (8 * pa))) ^ (inj << (8 * pa));
    if (pa > -4) return v ^ (inj >> (8 * -pa));
    return v;
}
// Bytes [16 - t, 16) of v cleared (t < 16).
__device__ __forceinline__ uint4 clear_high(uint4 v, uint32_t t) {
    const uint64_t mh = t >= 8 ? 0ull : ~0ull >> (8 * t);
    const uint64_t ml = t <= 8 ? ~0ull : ~0ull >> (8 * (t - 8));
    return make_uint4(v.x & (uint32_t)ml, v.y & (uint32_t)(ml >> 32), v.z & (uint32_t)mh, v.w & (uint32_t)(mh >> 32));
}
// M_t(v) for t < 16: t zero bytes through this lane's replicated slice-by-4
// tables (t / 4 dword steps, then byte steps on T0).
__device__ __forceinline__ uint32_t zeros_lds(uint32_t v, uint32_t t, const LaneCtx &c) {
    for (uint32_t q = 0; q < (t >> 2); ++q) v = step4_next(v, 0u, c);
    for (uint32_t r = 0; r < (t & 3u); ++r)
        v = lds_ld(kAux4Bytes + 0x10000u + ((v & 0xffu) << 8) + 128u + c.lane4) ^ (v >> 8);
    return v;
}

struct ItemBuf {
    K1Regs d;     // the window, in K1's lane layout (pieces 512 k + 16 li)
    uint32_t st;  // its image: t | kStFused | kStSane | kStValid
};

template <int MODE, bool OFFS>
__global__ __launch_bounds__(1024) void k_lines(SpanArgs a, const uint4 *__restrict__ img, ItemsOut io) {
    // MODE 0: equal spans of a.len bytes by offsets (OFFS) or stride, MODE 1/2/3:
    // item images (verify / stamp / stamp that keeps carried CRCs) by offsets
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint64_t n = a.n;
    const uint64_t nsr = io.nsr;
    const uint64_t run_imgs = 2ull * nsr;
    const uint64_t waves = blockDim.x >> 6;
    const uint64_t W = gridDim.x * waves;
    const uint64_t w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (uint32_t)waves + (threadIdx.x >> 6));
    // Runs, dealt round robin (round 5): run k of wave w is the images
    // [(k W + w) 2 nsr, +2 nsr), so at any time the waves' windows lie
    // within W runs (~1 GB at 4165-B images) of each other.  Round 4 gave
    // each wave a contiguous chunk of ceil(n / W) images with staggered
    // first runs (-2.5 % at 300 pages); at 1000 pages (67 GB) those 4096
    // streams, 16 MB apart, ran 3.5-7 % slower per page than 300 pages did,
    // and the round-robin order took config 5 at 1000 pages from
    // 11.32-11.76 to 10.92-10.93 ms, 300 pages and config 2r level or better
    // (profiles/r05_ablations/k5_run_order_ab.txt).
    // tests/test_items_lines_model.py checks that the runs cover every image
    // exactly once.
    auto run_start = [&](uint64_t k) -> uint64_t { return (k * W + w0) * run_imgs; };
    if ((uint64_t)blockIdx.x * waves * run_imgs >= n) return;
    if (MODE != 0 && io.route && *io.route == 0) {  // the census sent the batch to the planned path
        if (blockIdx.x == 0 && threadIdx.x == 0) *io.nfb = (uint32_t)n;
        return;
    }
    load_tables(smem, img, kLdsImageK1Bytes);
    if (run_start(0) >= n) return;
    const uint32_t lane = threadIdx.x & 63u, li = lane & 31u, g = lane >> 5;
    const LaneCtx c = make_lane_ctx(li);
    gbyte *const gb = (gbyte *)a.base;
    gbyte *const gz = (gbyte *)zero_slot(a);
    const uint32_t base_lo = (uint32_t)(uintptr_t)a.base;  // (alignments: the offsets are from a.base)
    uint32_t nb = 0;  // bad (malformed or mismatching) images seen by this lane

    // (r: the wave's round, 0, 1, 2, ...)
    auto item_of = [&](uint64_t r) -> uint64_t { return run_start(r) + lane; };
    auto valid_of = [&](uint64_t r) { return lane < 2 * nsr && item_of(r) < n; };
    auto off_of = [&](uint64_t r) -> uint64_t {
        // (offsets or stride is a template choice: a load on one side of a
        // branch leaves the waitcnt pass a merged state that waits for it)
        return valid_of(r) ? (OFFS ? a.offsets[item_of(r)] : item_of(r) * a.stride) : 0;
    };
    // MODE 0: x^(-8 (t + 128)), t < 16, lane-distributed (lane j holds t = j & 15)
    const uint32_t xinv = MODE == 0 ? mulmodp_dev(a.xpow[kXpowInv + (lane & 15u)], io.xm128) : 0u;
    uint64_t noff = off_of(0);  // this lane's image offset in the wave's next run
    uint32_t ncin = MODE == 0 && a.crc_in && valid_of(0) ? a.crc_in[item_of(0)] : 0u;

    // this lane's image of the run
    uint32_t eglo = 0, eghi = 0, est = 0;  // window start A (offset from a.base), status
    uint32_t p_kh = 0, p_inj = ~0u, p_stored = 0, p_nh = 0, p_nt = 0, p_eta = 0;
    uint64_t p_pho = 0, p_b = 0;
    uint32_t r_h = 0, r_t = 0, er = 0;
    uint4 pc[kHeadPieces], tc[kTailPieces];
    auto prep_head = [&](uint64_t r) {
        const bool valid = valid_of(r);
        const uint64_t off = noff;
        ItemHdr h{0u, 0u, 0u, 0u};
        ItemDesc it{a.base, 0u, 0u, false};
        p_inj = ~0u;  // ~c: the register's initial value, XORed in at p
        if (MODE == 0) {
            it.sane = valid && off <= a.base_bytes && a.len <= a.base_bytes - off;
            it.len = a.len;
            if (a.crc_in) p_inj = ~ncin;
        } else {
            const bool hdr_ok = valid && off + 48 <= a.base_bytes;
            if (hdr_ok) h = parse_hdr(gb + off);
            it = item_desc(a, off, h, hdr_ok);
        }
        p_stored = h.exptime;
        const uint32_t len = it.sane ? it.len : 0u;
        const uint64_t po = MODE == 0 ? off : off + 32;  // span start (offset)
        const uint64_t pe = po + len;                     // span end
        const uint32_t pa = base_lo + (uint32_t)po, ea = base_lo + (uint32_t)pe;
        const uint64_t A = po + 4 + ((0u - (pa + 4u)) & (kLineBytes - 1));
        const uint64_t B = pe - (ea & (kLineBytes - 1));
        const uint32_t pad = (0u - ea) & (kTailAlign - 1);
        const bool fused = it.sane && len >= 4 && lines_fused((int64_t)B - (int64_t)A);
        p_kh = pa & 15u;
        p_pho = po - p_kh;
        p_b = B;
        p_nh = fused ? (uint32_t)(A - p_pho) >> 4 : 0u;
        p_nt = fused ? (uint32_t)(pe + pad - B) >> 4 : 0u;
        p_eta = (uint32_t)(pe + pad - A);  // Et - A
        eglo = (uint32_t)A;
        eghi = (uint32_t)(A >> 32);
        est = pad | (fused ? kStFused : 0u) | (it.sane ? kStSane : 0u) | (valid ? kStValid : 0u) |
              (fused && B - A < kBlockBytes ? kSt31 : 0u);
    };
    auto head_loads = [&]() {
#pragma unroll
        for (uint32_t k = 0; k < kHeadPieces; ++k) pc[k] = ld16(k < p_nh ? gb + p_pho + 16 * k : gz);
    };
    // r_h = register from ~c over [p, A): bytes below p cleared, ~c injected at p
    auto head_chain = [&]() {
        uint32_t x = 0;
#pragma unroll
        for (uint32_t k = 0; k < kHeadPieces; ++k) {
            const uint32_t w[4] = {pc[k].x, pc[k].y, pc[k].z, pc[k].w};
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const int32_t pa = (int32_t)p_kh - (int32_t)(16 * k + 4 * j);
                const uint32_t d = head_dword(w[j], pa, p_inj);
                const uint32_t nx = (k == 0 && j == 0) ? d : step4_next(x, d, c);
                x = k < p_nh ? nx : x;
            }
        }
        r_h = p_nh ? step4_next(x, 0u, c) : 0u;
    };
    // (the last piece's bytes from E on are cleared: pad of them)
    auto tail_loads = [&]() {
#pragma unroll
        for (uint32_t k = 0; k < kTailPieces; ++k) tc[k] = ld16(k < p_nt ? gb + p_b + 16 * k : gz);
    };
    auto tail_chain = [&]() {
        uint32_t x = 0;
#pragma unroll
        for (uint32_t k = 0; k < kTailPieces; ++k) {
            const uint4 v = k + 1 == p_nt ? clear_high(tc[k], est & 15u) : tc[k];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t nx = (k == 0 && j == 0) ? w[j] : step4_next(x, w[j], c);
                x = k < p_nt ? nx : x;
            }
        }
        r_t = p_nt ? step4_next(x, 0u, c) : 0u;
    };
    // Loads of step s into b: its window and its status.  Past the run
    // (s >= ns: the prefetch of the run's last step, whose result is not
    // used) the window is the workgroup's zero slot, in L2: a repeat of the
    // run's last window fetched it from HBM again (non-temporal loads), one
    // step in 1 + nsr, 3 % of config 5's bytes.  K1's layout
    // and policy (round 5): lane li holds the window's 16-B pieces at
    // 512 k + 16 li, each instruction reads whole lines, non-temporal (the
    // window's lines are read by nothing else: the heads and tails lie
    // outside [A, B)): config 2r 0.743-0.766 -> 0.693-0.694 ms, config 5
    // 3.58-3.59 -> 3.50 ms and stamp 3.85-3.86 -> 3.75-3.76 ms per 300 pages
    // (profiles/r05_ablations/k5_lines_pieces_nt_ab.txt).
    auto ld = [&](ItemBuf &b, uint32_t s, uint32_t ns) {
        const int src = (int)(2 * min(s, ns - 1) + g);
        const uint64_t lo = (uint32_t)__shfl((int)eglo, src, 64), hi = (uint32_t)__shfl((int)eghi, src, 64);
        b.st = (uint32_t)__shfl((int)est, src, 64);
        const bool real = s < ns;  // (wave-uniform)
        gbyte *blk = ((b.st & kStFused) && real ? gb + (lo | (hi << 32)) : gz) + 16 * li;
        const bool z7 = (b.st & kSt31) && real && li >= 24u;  // piece 7 past B (the window's last line): zeros
#pragma unroll
        for (int k = 0; k < (int)kK1Pieces - 1; ++k) b.d.d[k] = ld16_nt(blk + k * kK1Piece);
        b.d.d[kK1Pieces - 1] = ld16_nt(z7 ? gz + 16 * li : blk + (kK1Pieces - 1) * kK1Piece);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto part0 = [&](ItemBuf &b) { return reduce_level<0>(k1_lane_value(b.d, c), (lane & 1u) == 0u); };
    // The epoch lanes collect R of their images from the lanes that finished
    // them (steps s0 .. s0 + cnt - 1 in lanes 0 .. cnt - 1 of each group).
    auto collect = [&](uint32_t r, uint32_t s0, uint32_t cnt) {
        const uint32_t sl = lane >> 1;
        const int src = (int)((lane & 1u) * 32u + (sl - s0));
        const uint32_t v = (uint32_t)__shfl((int)r, sl - s0 < cnt ? src : 0, 64);
        er = sl - s0 < cnt ? v : er;
    };
    // End of a run: every epoch lane finishes its image.
    auto finish_run = [&](uint64_t r) {
        const bool valid = valid_of(r);
        const uint64_t item = item_of(r);
        const bool fused = est & kStFused, sane = est & kStSane;
        const uint32_t pad = est & 15u;
        // (every lane: a lane-distributed value read under a branch would come
        // from lanes the branch left inactive)
        const uint32_t xt = MODE == 0 ? (uint32_t)__shfl((int)xinv, (int)pad, 64) : 0u;
        uint32_t v = 0;  // W = M_128(V) = M_{pad + 128}(f)
        if (fused) {
            const uint32_t dl = p_eta - (kBlockBytes - kLineBytes);  // d = Et - A - 3968
            uint32_t y = apply_op<4>(kAuxSpanFold, apply_op<4>(kAuxSpanFold, r_h)) ^ er;
            if (dl & 256u) y = apply_op<4>(kAuxTree + 12, apply_op<4>(kAuxTree + 12, y));
            if (dl & 128u) y = apply_op<4>(kAuxTree + 12, y);
            if (dl & 64u) y = apply_op<4>(kAuxTree + 8, y);
            if (dl & 32u) y = apply_op<4>(kAuxTree + 4, y);
            if (dl & 16u) y = apply_op<4>(kAuxTree, y);
            v = zeros_lds(y, dl & 15u, c) ^ apply_op<4>(kAuxTree + 12, r_t);
        }
        if (valid) {
            if (MODE == 0) {
                a.out[item] = fused ? ~mulmodp_dev(v, xt) : 0u;
                nb += !sane;  // (out of the buffer: not read, out 0, counted)
            } else if (MODE == 1) {
                if (fused || !sane) {
                    const bool good = fused && v == apply_op<4>(kAuxTree + 12, zeros_lds(~p_stored, pad, c));
                    a.ok[item] = good;
                    nb += !good;
                }
            } else {
                // MODE 3: a carried image (stored CRC != 0) is compared here as
                // a verify's and gets no record, so k_fix writes nothing for it
                const bool kept = fused && carried_image<MODE>(sane, p_stored);
                if (kept) {
                    const bool good = v == apply_op<4>(kAuxTree + 12, zeros_lds(~p_stored, pad, c));
                    if (a.ok) a.ok[item] = good ? kItemKept : 0;
                    nb += !good;
                }
                io.rt[item] = fused && !kept ? make_uint2(v, pad | kRtFused) : make_uint2(0u, 0u);
                if (!sane) {
                    if (a.ok) a.ok[item] = 0;
                    ++nb;
                }
            }
        }
        if (MODE != 0) {
            const bool fb = valid && sane && !fused;
            const uint64_t m = __ballot(fb);  // the fallback list: one atomic per wave with entries
            if (m) {
                const uint32_t first = (uint32_t)__ffsll((unsigned long long)m) - 1u;
                uint32_t base = 0;
                if (lane == first) base = atomicAdd(io.nfb, (uint32_t)__popcll(m));
                base = __shfl(base, (int)first, 64);
                if (fb) io.fb[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)item;
            }
        }
    };
    ItemBuf ra, rb;
    for (uint64_t r = 0; run_start(r) < n; ++r) {
        const uint64_t left = n - run_start(r);
        const uint32_t ns = (uint32_t)min(nsr, (left + 1) / 2);
        prep_head(r);
        // the head and tail lines of neighbouring images are the same lines:
        // both loads at once, so one image's tail and the next image's head
        // are fetched together (tail loads after the head chain came ~2 us
        // later and fetched the shared line again: 1.036x for config 2r)
        head_loads();
        tail_loads();
        __builtin_amdgcn_sched_barrier(0);  // (not sunk towards the tail chain)
        // the next run's offsets (and initial CRCs), consumed one run later
        noff = off_of(r + 1);
        if (MODE == 0) ncin = a.crc_in && valid_of(r + 1) ? a.crc_in[item_of(r + 1)] : 0u;
        head_chain();
        ld(ra, 0, ns);  // (after the head chain: its registers are free again)
        tail_chain();
        er = 0;
        uint32_t s = 0;
        for (; s + 4 <= ns; s += 4) {
            ld(rb, s + 1, ns);
            const uint32_t va = part0(ra);
            ld(ra, s + 2, ns);
            const uint32_t vb = part0(rb);
            const uint32_t vab = group_pair_level1(va, vb, lane);
            ld(rb, s + 3, ns);
            const uint32_t vc = part0(ra);
            ld(ra, s + 4, ns);
            const uint32_t vd = part0(rb);
            collect(group_reduce32_quad_span(vab, group_pair_level1(vc, vd, lane), lane), s, 4);
        }
        for (; s + 2 <= ns; s += 2) {
            ld(rb, s + 1, ns);
            const uint32_t va = part0(ra);
            ld(ra, s + 2, ns);
            const uint32_t vb = part0(rb);
            collect(group_reduce32_pair_span(va, vb, lane), s, 2);
        }
        if (s < ns) {
            // (part0 ran level 0; levels 1..4 of the span tree)
            collect(group_reduce32_single_span(part0(ra), lane), s, 1);
        }
        finish_run(r);
    }
    // one atomic per wave for the bad count
    wave_sum(nb);
    if (lane == 0 && nb) atomicAdd(a.nbad, (unsigned long long)nb);
}

// The last step of a K5 stamp (MODE 2/3), one thread per image: from W =
// M_{t + 128}(f), f the register after the span from ~0, the CRC is
// ~M_{-t-128}(W) (xm128 = x^(-8 * 128)), stamped into
// the image's exptime as the spill CRC (storage.c:567).  A separate pass:
// within k_lines an image's stamp could race with another wave's read of the
// same bytes when images overlap.  (MODE 0 spans get their CRC from the epoch
// lanes of k_lines itself, and so do MODE 3's carried images their verdict:
// they have no record here, so a wbuf of carried images costs no scattered
// 4-B store at all.)
__global__ void k_fix(SpanArgs a, const uint2 *rt, const uint32_t *route, uint32_t xm128) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    if (route && *route == 0) return;  // (k_lines took no image)
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 r = rt[i];
        if (r.y & kRtFused) {
            const uint32_t crc = ~mulmodp_dev(mulmodp_dev(r.x, xm128), a.xpow[kXpowInv + (r.y & 15u)]);
            uint8_t *p = const_cast<uint8_t *>(a.base) + a.offsets[i] + 32;
            // non-temporal: plain stores left 16 M dirty 32-B sectors in the
            // caches, written back while the next batch streamed (its
            // k_lines<2> 0.11 ms slower per 300 pages); so the write-backs
            // happen here (k_fix 0.17 -> 0.25 ms), stamp -1.2 % in all
            // (profiles/r04_ablations/k_fix_nontemporal_ab.txt)
            for (int b = 0; b < 4; ++b) __builtin_nontemporal_store((uint8_t)(crc >> (8 * b)), p - 4 + b);
            if (a.ok) a.ok[i] = 1;
        }
    }
}

// K5 or the planned path, decided on the device (round 4; it was the host's
// guess from the batch's average image size, which a mix of short and long
// images can match): the headers of up to kCensus images spread evenly over
// the batch, and *route = 1 when at least 15/16 of them have K5's shape (one
// 4 KiB block after a short head fragment).  Below that the images K5 leaves
// to its fallback cost a second pass, and the planned path takes the batch
// (k_lines then lists every image).  One workgroup, one header per thread.
constexpr uint32_t kCensus = 1024;
template <int MODE>
__global__ __launch_bounds__(kCensus) void k_census(SpanArgs a, uint32_t *route) {
    MCRC_VGPR_FLOOR();
    __shared__ uint32_t cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const uint64_t n = a.n, s = min(n, (uint64_t)kCensus);
    if (threadIdx.x < s) {
        const uint64_t i = threadIdx.x * n / s;
        const ItemDesc it = fetch_item<MODE>(a, i);
        const uint64_t pa = (uintptr_t)it.p, A = (pa + 4 + kLineBytes - 1) & ~(uint64_t)(kLineBytes - 1);
        const uint64_t B = (pa + it.len) & ~(uint64_t)(kLineBytes - 1);
        const bool fused = it.len >= 4 && lines_fused((int64_t)B - (int64_t)A);
        if (it.sane && fused) atomicAdd(&cnt, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) *route = 16ull * cnt >= 15ull * s ? 1u : 0u;
}

}  // namespace mcrc_dev
