// k_common.h -- what the kernel families share: the 16-B loads, the block and
// span geometry, SpanArgs, the per-thread byte-table chains (Tab8,
// reg_advance, span_corr), the item header parse, emit and count_bad.
#pragma once

#include "crc32c_device.h"
#include "k_consts.h"

namespace mcrc_dev {

// 16-B load of item bytes.  (The streaming reads of K1, K5 and the span
// kernels use ld16_nt below, since round 5 on whole lines; non-temporal
// loads of 16-B anchored blocks were 5-11 % worse in round 1.)
__device__ __forceinline__ uint4 ld16(const void *p) { return *reinterpret_cast<const uint4 *>(p); }
// Global-memory byte and piece pointers.  k_lines keeps its addresses in
// these: derived from the kernel arguments through generic pointers, they
// lost their address space to an optimizer freeze, and the flat loads that
// result also count in lgkmcnt (every LDS wait of the chains then waits for
// the block prefetch too).
typedef const __attribute__((address_space(1))) uint8_t gbyte;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld16(gbyte *p) {
    const u32x4 v = *(const __attribute__((address_space(1))) u32x4 *)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

// Non-temporal 16-B load (the `nt` policy bit: the line is streamed, not kept
// in L2 / the Infinity Cache).
__device__ __forceinline__ uint4 ld16_nt(const uint8_t *p) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint4 ld16_nt(gbyte *p) {
    const u32x4 v = __builtin_nontemporal_load((const __attribute__((address_space(1))) u32x4 *)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ uint32_t dw4(const uint4 &v, int k) {
    return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
}

// K1's lane layout (round 5).  A 32-lane group owns one 4096-B item, and lane
// i holds the 16-B pieces at 512 k + 16 i, k = 0..7: each load instruction
// reads 512 contiguous bytes per group (two items, 1 KiB per wave), so every
// 128-B line is read whole by one instruction.  With non-temporal loads that
// reads 4 GiB at 82-83 % of the HBM peak, against 73-76 % for the 32-B-per-
// lane rows of rounds 1-4 (lane i at 32 i + 16 q of each KiB, two
// instructions per line) and 69-71 % for either shape with the default
// policy (profiles/r05_k1_ceiling.txt).  Algebra: the piece at 512 k + 16 i
// stands M_{512 (7-k) + 16 (31-i)} from the item's end.  Lane i runs one
// four-dword chain per piece; the chains of each half item fold through the
// shifted last steps M_1536, M_1024, M_512 (and the plain step), the first
// half moves up by M_2048, and the lane tree merges 16-B granules (levels
// M_16 .. M_128; level 4 = level 3 twice).  Table image: build_lds_image_span
// at chunk 16 (crc32c_gf2.h): tree at tables 0..15, M_2048 at 16..19, the
// shifted steps at kAuxShift2 / kAuxShift1 / kAuxShift0.  K1 itself holds
// half an item at a time (K1Half / k1_half_value, k_fixed.h); K4 and K5 hold
// the whole window (K1Regs / k1_lane_value, k_window.h), and the span kernel's
// blocks use the same layout (BlockWin, k_spans.h).
constexpr uint32_t kK1Pieces = 8, kK1Piece = 512;  // pieces per lane and item, their spacing
constexpr uint32_t kK1LaneBytes = 16;              // (the image's chunk)
static_assert(kK1Pieces * kK1Piece == 4096 && 32 * kK1LaneBytes == kK1Piece, "K1 covers a 4 KiB item");

// Pieces as they lie (K2/K3, and what span_corr below corrects for; the work
// units and their geometry: k_spans.h).  A span D = [p, E) is read as the 16-B aligned pieces
// [ph, Ea), ph = p rounded down to 16 and Ea = E rounded up to a 128-B line
// (grid_pad, round 5; 16 before), the head's foreign bytes F_h = [ph, p)
// included and the tail's F_t = [E, Ea) cleared in registers (the last line
// of the span's last block, mask_tail; round 5): the span kernel computes
// R = raw([ph, E) followed by t = |F_t| zeros) with no initial value.  The
// algebra of crc32c.c:58-137 gives
//   R = M_{|D|+t}(raw(F_h)) ^ M_t(raw(D)), so
//   crc32c(c, D) = ~M_{-t}(R ^ Z),   Z = M_{|D|+t}(~c ^ raw(F_h)).
// Z depends only on c and the at most 15 bytes of F_h, which share the head
// piece (and for item images the header's line), so one thread per span
// computes it (span_corr: k_count before the span kernel, or k_final after
// it), at a thirty-second of the cost of doing it in a 32-lane group; the
// span kernel's per-unit work is its lane reduction and one store.  (Until
// round 5 the thread also read F_t and XORed raw(F_t) into Z: a line per
// span that the span kernel reads again.)

constexpr uint32_t kWhole = 0xffffffffu;      // unit segment index: the whole span
// Pieces outside a span are read from a zeroed buffer; workgroup b reads the
// 16 B at zero + 4 KiB * (b % 256), so the workgroups' zero reads spread over
// L2 channels instead of all landing on one line (cf. K1's last prefetch).
constexpr uint32_t kZeroSlots = 256;
constexpr uint64_t kZeroBytes = 4096ull * kZeroSlots;

// Rows of the shift table (SpanArgs::segpow) below its second-factor rows:
// units ending less than 16 MiB before their span's end take one multiply.
constexpr uint32_t kSegpowLo = 4096;

struct SpanArgs {
    const uint8_t *base;       // all spans live in [base, base + base_bytes)
    uint64_t base_bytes;
    const uint64_t *offsets;   // span i starts at base + offsets[i] (MODE 0)
                               // or item image i at base + offsets[i] (MODE 1)
    uint64_t stride;           // when offsets == nullptr: base + i * stride
    const uint32_t *lens;      // per-span lengths, or nullptr: every span is `len`
    uint32_t len;
    const uint32_t *crc_in;    // MODE 0: per-span initial CRC or nullptr (0)
    uint32_t *out;             // MODE 0: CRC per span
    uint8_t *ok;               // MODE 1: 1 if the stored CRC matches; MODE 2/3 (optional): kItemStamped,
                               // MODE 3: kItemKept for a carried image whose stored CRC matches
    unsigned long long *nbad;  // MODE 1/2/3: count of mismatches / malformed images;
                               // MODE 0: spans outside [base, base + base_bytes) (atomic)
    uint64_t n;                // spans (items)
    const uint32_t *xpow;      // x^(8*j), x^(8*1024*j), x^(8*2^20*j) (3 x 1024), x^(-8t) (16),
                               // x^(8*2^30*j) (8): layout kXpow*
    const uint32_t *tab8;      // 16 x 256 byte tables (Tab8)
    const uint4 *zero;         // kZeroBytes of zeros in device memory
    // work units (nullptr: unit u = span u, one segment)
    const struct UnitRec *units;
    const uint32_t *nunits;    // device-side unit count
    uint32_t *span_acc;        // planned batches: R per span (segment units XOR their shifted values in)
    const uint32_t *segpow;    // rows k (x^i * x^(8 * 4096 * k), i < 32) for k < kSegpowLo, then k = kSegpowLo j
    const uint32_t *starts;    // balanced plan: share v's records are [starts[v], starts[v + 1])
                               // (0xffffffff: *nunits); nullptr: round robin over units
    uint32_t rounds;           // balanced plan: group g takes shares g, G + g, .. (rounds of them)
    uint64_t region;           // MODE 1: items never cross a multiple of `region` (0: no bound)
    uint32_t cfl;              // MODE 1/2: bytes of the ITEM_CFLAGS suffix, sizeof(client_flags_t):
                               // 4, or 8 in a LARGE_CLIENT_FLAGS build (memcached.h:96-100)
    // k_small only (nullptr: nbad is the caller's to zero and read): the last
    // workgroup moves *nbad to this pinned host word and zeroes *nbad and *done
    unsigned long long *host_nbad;
    uint32_t *done;            // finished workgroups
    // planned path over a list whose length is known only on the device (K5's
    // fallback list): n spans at most, *dn of them (nullptr: n)
    const uint32_t *dn;
};

__device__ __forceinline__ uint64_t span_count(const SpanArgs &a) { return a.dn ? (uint64_t)*a.dn : a.n; }
// This workgroup's slot of the zeroed buffer (kZeroSlots).
__device__ __forceinline__ const uint4 *zero_slot(const SpanArgs &a) {
    return a.zero + (blockIdx.x % kZeroSlots) * (4096 / 16);
}

struct ItemDesc {
    const uint8_t *p;
    uint32_t len;
    uint32_t aux;  // MODE 0: initial CRC; MODE 1/2/3: stored CRC
    bool sane;     // MODE 1/2/3: header parsed to an in-bounds span
};

// t = Ea - E: a span's grid ends at Ea = E rounded up to 16.  (Rounding up to
// a 128-B line makes every block whole lines -- a 16-B anchored block fetches
// 33 lines per 4 KiB -- and the span kernel 1.6-2.4 % faster, but the span's
// thread then reads and folds up to 127 foreign bytes: k_count +40 %, k_final
// +57 %, a net loss on configs 2r and 5.)
constexpr uint32_t kTailAlign = 16;
__device__ __forceinline__ uint32_t tail_pad(const uint8_t *p, uint32_t len) {
    return (uint32_t)(-(uintptr_t)(p + len)) & (kTailAlign - 1);
}
__device__ __forceinline__ uint32_t grid_pad(const uint8_t *p, uint32_t len) {
    return (uint32_t)(-(uintptr_t)(p + len)) & (kGridAlign - 1);
}

// Segments of a virtual span of vlen bytes, anchored at Ea; the head segment
// keeps the remainder (17 B up to kSegBytes + 16 B).
__device__ __forceinline__ uint32_t nseg_of(uint32_t vlen) {
    return vlen <= kSegBytes + 16 ? 1u : (vlen - 16 + kSegBytes - 1) / kSegBytes;
}

// Layout of the x^(8n) table (SpanArgs::xpow).
constexpr uint32_t kXpowInv = 3072;                // x^(-8t), t < kGridAlign
constexpr uint32_t kXpowL3 = kXpowInv + kGridAlign;  // x^(8 * 2^30 * j), j < 8
constexpr uint32_t kXpowDwords = kXpowL3 + 8;

// x^(8n) mod P (n < 2^33): one to four table entries multiplied.
__device__ __forceinline__ uint32_t xpow8_dev(const uint32_t *xp, uint64_t n) {
    uint32_t r = xp[n & 1023u];
    if (n >> 10) r = mulmodp_dev(r, xp[1024 + ((n >> 10) & 1023u)]);
    if (n >> 20) r = mulmodp_dev(r, xp[2048 + ((n >> 20) & 1023u)]);
    if (n >> 30) r = mulmodp_dev(r, xp[kXpowL3 + (uint32_t)(n >> 30)]);
    return r;
}

// A 16-B piece as two little-endian halves.
struct Piece {
    uint64_t lo, hi;
};
__device__ __forceinline__ Piece ld_piece(const uint8_t *p) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    return {v.x | ((uint64_t)v.y << 32), v.z | ((uint64_t)v.w << 32)};
}
__device__ __forceinline__ Piece ld_piece(gbyte *p) {
    const uint4 v = ld16(p);
    return {v.x | ((uint64_t)v.y << 32), v.z | ((uint64_t)v.w << 32)};
}
// Bytes moved s positions up (s <= 16), zeros shifted in.
__device__ __forceinline__ Piece shl_bytes(Piece v, uint32_t s) {
    if (s >= 16) return {0, 0};
    if (s >= 8) return {0, v.lo << (8 * (s - 8))};
    if (s == 0) return v;
    return {v.lo << (8 * s), (v.hi << (8 * s)) | (v.lo >> (64 - 8 * s))};
}
// Byte tables in LDS for the per-thread work of k_count / k_final: T_j[b] =
// the register after byte b followed by j zero bytes, j < 16 (T_0 is
// crc32c.c:399's byte-wise table crc32c_table_little[0]; crc32c.c:401-415 uses
// eight of them).  A whole 16-B piece is one step of 16 independent lookups:
// only the four that read the running register depend on the previous step,
// so a thread's chain is one LDS latency per 16 bytes.  (A dword per step
// took 0.21 ms of k_count on config 3, a copy of one table per bank with four
// dependent lookups per dword 0.45 ms: the per-thread chains are
// latency-bound, not conflict-bound.)
struct Tab8 {
    const uint32_t *s;  // T_j at s + 256 j
    __device__ __forceinline__ uint32_t T(uint32_t j, uint32_t b) const { return s[256 * j + b]; }
    // the register r advanced over the 16 bytes of v
    __device__ __forceinline__ uint32_t piece(uint32_t r, Piece v) const {
        const uint32_t x = r ^ (uint32_t)v.lo, d1 = (uint32_t)(v.lo >> 32), d2 = (uint32_t)v.hi,
                       d3 = (uint32_t)(v.hi >> 32);
        return (T(15, x & 255u) ^ T(14, (x >> 8) & 255u) ^ T(13, (x >> 16) & 255u) ^ T(12, x >> 24)) ^
               (T(11, d1 & 255u) ^ T(10, (d1 >> 8) & 255u) ^ T(9, (d1 >> 16) & 255u) ^ T(8, d1 >> 24)) ^
               (T(7, d2 & 255u) ^ T(6, (d2 >> 8) & 255u) ^ T(5, (d2 >> 16) & 255u) ^ T(4, d2 >> 24)) ^
               (T(3, d3 & 255u) ^ T(2, (d3 >> 8) & 255u) ^ T(1, (d3 >> 16) & 255u) ^ T(0, d3 >> 24));
    }
    // M_4096(r): operator tables 16..19 (slice k: M_4096 of byte b at bits 8k)
    __device__ __forceinline__ uint32_t block(uint32_t r) const {
        return (T(16, r & 255u) ^ T(17, (r >> 8) & 255u)) ^ (T(18, (r >> 16) & 255u) ^ T(19, r >> 24));
    }
    // M_n(r): the register r advanced over n zero bytes, 0 <= n <= 16
    __device__ __forceinline__ uint32_t zeros(uint32_t r, uint32_t n) const {
        if (n >= 4)
            return T(n - 1, r & 255u) ^ T(n - 2, (r >> 8) & 255u) ^ T(n - 3, (r >> 16) & 255u) ^ T(n - 4, r >> 24);
        uint32_t z = n == 0 ? r : r >> (8 * n);  // the bytes not yet shifted out
        for (uint32_t k = 0; k < n; ++k) z ^= T(n - 1 - k, (r >> (8 * k)) & 255u);
        return z;
    }
};
constexpr uint32_t kTab8Dwords = 20 * 256;  // 16 byte tables + the M_4096 operator, 20 KiB
// (every thread of the block calls it)
// (s: 16-B aligned; 16-B pieces, every load of a thread issued before its
// stores, as load_tables)
__device__ __forceinline__ Tab8 load_tab8(uint32_t *s, const uint32_t *tab8) {
    constexpr uint32_t n = kTab8Dwords / 4, U = 8;
    uint4 *dst = reinterpret_cast<uint4 *>(s);
    const uint4 *src = reinterpret_cast<const uint4 *>(tab8);
    for (uint32_t i0 = threadIdx.x; i0 < n; i0 += U * blockDim.x) {
        uint4 v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) v[u] = src[min(i0 + u * blockDim.x, n - 1)];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) dst[min(i0 + u * blockDim.x, n - 1)] = v[u];
    }
    __syncthreads();
    return {s};
}

// Register after the 16 bytes of v from a zero register.
__device__ __forceinline__ uint32_t raw16(Piece v, const Tab8 &t) { return t.piece(0u, v); }

// Bytes [0, k) of v cleared.
__device__ __forceinline__ Piece clear_below(Piece v, uint32_t k) {
    const Piece m = shl_bytes({~0ull, ~0ull}, k);
    return {v.lo & m.lo, v.hi & m.hi};
}

// Register r advanced over the n bytes at p (one thread), one step per 16-B
// piece: a partial first or last piece is moved to the top of a zeroed piece
// (leading zeros leave a zero register unchanged), so
//   r' = M_m(r) ^ raw16(the m bytes at the top).
// Every load is an aligned piece holding a byte of [p, p + n).
constexpr int kAdvUnroll = 4;  // (8 and 16 measured slower: profiles/r04_ablations/k_count_unroll_ab.txt)
__device__ __forceinline__ uint32_t reg_advance(uint32_t r, const uint8_t *p, uint32_t n, const Tab8 &t) {
    if (n == 0) return r;
    const uint32_t kh = (uint32_t)((uintptr_t)p & 15u);
    const uint8_t *q = p - kh;
    if (kh + n <= 16u) {  // inside one piece: bytes [kh, kh + n)
        const Piece v = shl_bytes(ld_piece(q), 16u - kh - n);
        return t.zeros(r, n) ^ raw16(clear_below(v, 16u - n), t);
    }
    if (kh) {  // bytes [kh, 16) of the first piece
        r = t.zeros(r, 16u - kh) ^ raw16(clear_below(ld_piece(q), kh), t);
        n -= 16u - kh;
        q += 16;
    }
#pragma unroll kAdvUnroll
    for (; n >= 16; n -= 16, q += 16) r = t.piece(r, ld_piece(q));
    if (n) r = t.zeros(r, n) ^ raw16(shl_bytes(ld_piece(q), 16u - n), t);  // bytes [0, n) of the last piece
    return r;
}

// Head fragment.  The block grid of a span is anchored at Ea, 4 KiB apart
// (segments are whole numbers of blocks, so every unit of the span uses the
// same grid); G1 = the first grid point after ph.  The span kernel would
// spend a whole block step of its group on [p, G1), mostly on rows without a
// byte of the span; when G1 - p <= kFragMax the span's thread takes those
// bytes instead (reg_advance), the head unit starts at G1, and a span whose
// virtual length is at most kWholeMax is not given to the span kernel at all.
// (The limits are measured: a thread's chain is serial, one LDS round trip
// per 16 B, so long fragments cost more than the block step they save --
// DESIGN.md section 3.)
static_assert(kWholeMax + kGridAlign <= kBlockBytes, "a whole span held by its thread is its own fragment (G1 = Ea)");
struct SpanHead {
    uint64_t g1o;  // G1 - p
    bool drop;     // [p, G1) is the thread's
};
__device__ __forceinline__ SpanHead span_head(const uint8_t *p, uint32_t len) {
    const uint64_t kh = (uintptr_t)p & 15u;
    const uint64_t x = (uint64_t)len + grid_pad(p, len) + kh;  // Ea - ph
    const uint64_t g1o = x - kBlockBytes * ((x - 1) / kBlockBytes) - kh;
    return {g1o, frag_drop(len, g1o, x - kh)};
}

// One-block geometry of span [p, p + len): true if its unit is one whole block
// (at G1 when its head fragment is the thread's, else at ph; *g1 = the block),
// or it has no unit at all (*none); false: neither.
__device__ __forceinline__ bool one_block(const uint8_t *p, uint32_t len, const uint8_t **g1, bool *none) {
    const uint64_t kh = (uintptr_t)p & 15u;
    const uint64_t vlen = (uint64_t)len + grid_pad(p, len);  // (64-bit: len may be close to 2^32)
    const uint64_t x = vlen + kh;  // Ea - ph
    const uint64_t g1o = x - kBlockBytes * ((x - 1) / kBlockBytes) - kh;
    const bool drop = frag_drop(len, g1o, vlen);
    *none = len == 0 || (drop && g1o == vlen);
    if (!drop && x == kBlockBytes) {  // the unit [ph, Ea) is itself one block
        *g1 = p - kh;
        return true;
    }
    *g1 = p + g1o;
    return *none || (drop && vlen - g1o == kBlockBytes);
}

// Z of span [p, p + len) with initial CRC c (see "Pieces as they lie"), for
// the R that the span kernel computes over the span's units (F_t cleared):
// - no bytes: the kernel reads nothing (R = 0), Z = M_t(~c);
// - head fragment taken (span_head): the kernel reads [G1, Ea), so
//   Z = M_{Ea-G1}(r) with r = the register from ~c over [p, G1),
//   or, when G1 = Ea, Z = M_t(register from ~c over D);
// - otherwise Z = M_{len+t}(~c ^ raw(F_h)): raw(F_h) = raw of the head
//   piece's first kh bytes moved to its top (leading zeros leave a zero
//   register unchanged).
// One thread.  (`pieces`: the third case whatever the head -- k_count's
// wave-cooperative whole spans, whole_chunks, whose R covers [ph, Ea).)
//
// Z as a register y to be moved up by N bytes: Z = M_N(y).  Every case of
// span_corr is of this form, so a wave whose spans take different cases
// (a head fragment taken or not) runs the multiply by x^(8N) once, not once
// per case (round 5: in k_count the divergent cases each ran theirs).
struct CorrArg {
    uint32_t y;
    uint64_t N;
};
__device__ __forceinline__ CorrArg span_corr_arg(const uint8_t *p, uint32_t len, uint32_t c, const Tab8 &t8,
                                                 bool pieces) {
    const uint32_t t = grid_pad(p, len);
    if (len == 0) return {~c, t};
    const uint64_t vlen = (uint64_t)len + t;
    const SpanHead h = span_head(p, len);
    if (pieces || !h.drop) {
        // the kernel's R covers the pieces [ph, Ea): y = ~c ^ raw(F_h), N = len + t
        const uint32_t kh = (uint32_t)((uintptr_t)p & 15u);
        uint32_t y = ~c;
        if (kh) y ^= raw16(shl_bytes(ld_piece(p - kh), 16 - kh), t8);  // raw(F_h)
        return {y, vlen};
    }
    // the head fragment [p, G1) is the thread's; G1 = Ea: the whole span,
    // whose register moves up by t
    const bool all = h.g1o == vlen;
    return {reg_advance(~c, p, all ? len : (uint32_t)h.g1o, t8), all ? (uint64_t)t : vlen - h.g1o};
}
__device__ __forceinline__ uint32_t corr_apply(const CorrArg &z, const Tab8 &t8, const uint32_t *xp) {
    // (one block, every one-block span: a table step)
    return z.N == kBlockBytes ? t8.block(z.y) : mulmodp_dev(z.y, xpow8_dev(xp, z.N));
}
__device__ __forceinline__ uint32_t span_corr(const uint8_t *p, uint32_t len, uint32_t c, const Tab8 &t8,
                                              const uint32_t *xp) {
    return corr_apply(span_corr_arg(p, len, c, t8, false), t8, xp);
}

// Item header fields (memcached.h:613-636) from bytes 28..43 of the image at
// it, read as the two aligned pieces holding them (every byte of those pieces
// shares its 16-B granule with a header byte, so no read leaves the image's
// pages).  ITEM_ntotal as memcached.h:149-152.
struct ItemHdr {
    uint32_t exptime;  // bytes 28..31: the spill CRC (storage.c:567)
    uint32_t nbytes;   // 32..35
    uint32_t flags;    // it_flags, 38..39
    uint32_t nkey;     // 41
    // cfl = sizeof(client_flags_t) (SpanArgs::cfl)
    __device__ __forceinline__ uint64_t ntotal(uint32_t cfl) const {
        return 48ull + nkey + 1 + nbytes + ((flags & 256u) ? cfl : 0) + ((flags & 2u) ? 8 : 0);
    }
};
//
// The fields are funnelled out of the pieces' dwords with v_alignbyte_b32, not
// with 64-bit shifts: a v_lshlrev_b64 whose shift amount sits in the last VGPR
// of the wave's allocation computes wrongly beside a co-resident wave on
// gfx950 (tools/shift64_top_vgpr.hip), and the 64-bit funnel
// this parse used through round 5 put its amount exactly there in a 24-VGPR
// kernel.  tests/test_kernel_resources.py checks that no kernel of the
// library, and no instruction of this parse, takes that form.
template <typename BytePtr>
__device__ __forceinline__ ItemHdr parse_hdr(BytePtr it) {
    // (pointer arithmetic, not an integer round trip: the loads stay global
    // loads instead of flat ones, which would also count in lgkmcnt)
    const uint32_t sh = (uint32_t)((uintptr_t)(it + 28) & 15u);  // 0..15
    const BytePtr q = it + 28 - sh;
    const bool two = sh + 13 >= 16;  // byte 41 lies in the next piece
    const Piece v0 = ld_piece(q), v1 = ld_piece(q + (two ? 16 : 0));
    const uint32_t d[8] = {(uint32_t)v0.lo, (uint32_t)(v0.lo >> 32), (uint32_t)v0.hi, (uint32_t)(v0.hi >> 32),
                           two ? (uint32_t)v1.lo : 0u, two ? (uint32_t)(v1.lo >> 32) : 0u,
                           two ? (uint32_t)v1.hi : 0u, two ? (uint32_t)(v1.hi >> 32) : 0u};
    // w[m] = the dword holding image byte 28 + 4m (and the next one's low bytes)
    const uint32_t qi = sh >> 2, b = sh & 3u;
    uint32_t w[5];
#pragma unroll
    for (uint32_t m = 0; m < 5; ++m) w[m] = qi == 0 ? d[m] : qi == 1 ? d[m + 1] : qi == 2 ? d[m + 2] : d[m + 3];
    // image bytes 28..31, 32..35, 36..39 (it_flags 38..39), 40..43 (nkey 41)
    const uint32_t o0 = __builtin_amdgcn_alignbyte(w[1], w[0], b), o1 = __builtin_amdgcn_alignbyte(w[2], w[1], b),
                   o2 = __builtin_amdgcn_alignbyte(w[3], w[2], b), o3 = __builtin_amdgcn_alignbyte(w[4], w[3], b);
    return {o0, o1, (o2 >> 16) & 0xffffu, (o3 >> 8) & 0xffu};
}

// The CRC span of the item image at base + off with header h (parsed when
// hdr_ok): [off + 32, off + ITEM_ntotal) (STORE_OFFSET, storage.h:43), the
// stored CRC in aux.
__device__ __forceinline__ ItemDesc item_desc(const SpanArgs &a, uint64_t off, const ItemHdr &h, bool hdr_ok) {
    ItemDesc d;
    const uint64_t ntotal = h.ntotal(a.cfl);
    d.aux = h.exptime;
    // an item never crosses its write buffer (extstore.c:627-636), so a
    // header claiming otherwise is corrupt
    const bool in_region = a.region == 0 || off / a.region == (off + ntotal - 1) / a.region;
    d.sane = hdr_ok && h.nkey != 0 && h.nbytes < 0x80000000u && ntotal - 32 <= kMaxSpan &&
             off + ntotal <= a.base_bytes && in_region;
    d.p = a.base + off + 32;
    d.len = d.sane ? (uint32_t)(ntotal - 32) : 0u;
    return d;
}

template <int MODE>
__device__ __forceinline__ ItemDesc fetch_item(const SpanArgs &a, uint64_t i) {
    const uint64_t off = a.offsets ? a.offsets[i] : i * a.stride;
    if (MODE == 0) {
        // a span outside [base, base + base_bytes) is not read (out = 0, counted)
        ItemDesc d;
        const uint32_t len = a.lens ? a.lens[i] : a.len;
        d.sane = off <= a.base_bytes && len <= a.base_bytes - off && len <= kMaxSpan;
        d.p = a.base + (d.sane ? off : 0);
        d.len = d.sane ? len : 0u;
        d.aux = a.crc_in ? a.crc_in[i] : 0u;
        return d;
    }
    const bool hdr_ok = off + 48 <= a.base_bytes;
    ItemHdr h{0u, 0u, 0u, 0u};
    if (hdr_ok) h = parse_hdr(a.base + off);
    return item_desc(a, off, h, hdr_ok);
}

// Item record written by k_count: {offset of the span (lo, hi | flags), len, z}:
// z = Z (span_corr; MODE 0 and 2) or, for a verify (MODE 1), W = Z ^ M_t(~stored CRC),
// so that the stored CRC matches iff R == W.  A keep-stamped stamp (MODE 3)
// decides per image: W and kCarried for a carried image (stored CRC != 0),
// Z for a fresh one.  The flags sit in the offset's top bits (rec_off).
constexpr uint32_t kInsane = 0x80000000u;   // !sane
constexpr uint32_t kCarried = 0x40000000u;  // MODE 3: verified, not stamped
constexpr uint32_t kRecFlags = kInsane | kCarried;
__device__ __forceinline__ uint64_t rec_off(const uint4 &r) { return r.x | ((uint64_t)(r.y & ~kRecFlags) << 32); }

// ok[] values of a stamp (CRC32C_ITEM_STAMPED / _KEPT, crc32c_batch.h).
constexpr uint8_t kItemStamped = 1, kItemKept = 2;
// MODE 3 (CRC32C_KEEP_STAMPED): an image whose stored CRC is not 0 was
// carried over with it (compaction, storage.c:1004-1006): compared, not
// stamped.
template <int MODE>
__device__ __forceinline__ bool carried_image(bool sane, uint32_t stored) {
    return MODE == 3 && sane && stored != 0u;
}

// Store (MODE 0) or stamp (MODE 2/3) the CRC of span `item`, which starts at p.
// Stamp writes the spill CRC into the image's exptime field, bytes 28..31 =
// p - 4 (storage.c:567), or into out[] when the caller stages the images (host
// path); ok[] (if any) marks stamped images.  A span that is not sane (outside
// the buffer, or a malformed image) was not read.  MODE 3 writes nothing for
// a carried image (stored: its exptime) and marks it kItemKept when crc equals
// the stored value.  Returns whether the caller counts the span as bad.
template <int MODE>
__device__ __forceinline__ bool emit(const SpanArgs &a, uint64_t item, uint32_t crc, bool sane, const uint8_t *p,
                                     uint32_t stored = 0u) {
    if (MODE == 0) {
        a.out[item] = sane ? crc : 0u;
    } else if (carried_image<MODE>(sane, stored)) {
        const bool good = crc == stored;
        if (a.ok) a.ok[item] = good ? kItemKept : 0;
        return !good;
    } else {
        if (a.ok) a.ok[item] = sane;
        if (!sane) return true;
        if (a.out) {
            a.out[item] = crc;
        } else {
            // one dword store at any alignment (global memory takes unaligned
            // stores on gfx950; the compiler emits that for this memcpy)
            __builtin_memcpy(const_cast<uint8_t *>(p) - 4, &crc, 4);
        }
    }
    return !sane;
}

// nb summed over the wave's 64 lanes, in every lane.
__device__ __forceinline__ void wave_sum(uint32_t &nb) {
    nb += __shfl_xor(nb, 1);
    nb += __shfl_xor(nb, 2);
    nb += __shfl_xor(nb, 4);
    nb += __shfl_xor(nb, 8);
    nb += __shfl_xor(nb, 16);
    nb += __shfl_xor(nb, 32);
}

// nbad += the per-thread counts of a workgroup: one atomic per workgroup.
// (Atomics on one address serialise in L2: one per bad item of a verify with
// 1 % corrupt items took 0.4 ms per 300 pages.)  Every thread of the block
// calls it.
__device__ __forceinline__ void count_bad(unsigned long long *nbad, uint32_t nb) {
    __shared__ uint32_t sum;
    if (threadIdx.x == 0) sum = 0;
    __syncthreads();
    wave_sum(nb);
    if (__lane_id() == 0 && nb) atomicAdd(&sum, nb);
    __syncthreads();
    if (threadIdx.x == 0 && sum) atomicAdd(nbad, (unsigned long long)sum);
}

}  // namespace mcrc_dev
