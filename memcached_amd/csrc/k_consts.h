// k_consts.h -- the geometry constants and the two shape predicates that the
// kernels and the host's routing (host_route.h) share.  Plain C++, no HIP
// include: a CPU program compiles the host's decisions against them.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MCRC_HD __host__ __device__ __forceinline__
#else
#define MCRC_HD static inline
#endif

namespace mcrc_dev {

// K1 geometry: a 32-lane group owns one 4096-B item, a wave two items per
// step.
constexpr uint32_t kK1Bytes = 4096;
// K1's lockstep rounds: every kK1RoundSteps steps (a multiple of 4: K1's main
// loop takes 4 steps a pass) the waves of a workgroup meet at a bare
// workgroup barrier, so that they finish together and the CU keeps its full
// load depth until its ranges are done.  4, 8, 16 and 32 alternated with the
// barrier-free loop on one box: 0.6314, 0.6390, 0.6394, 0.6431 against
// 0.6557 ms per headline launch (profiles/k1_lockstep_ab.jsonl).
constexpr uint32_t kK1RoundSteps = 4;
static_assert(kK1RoundSteps >= 4 && kK1RoundSteps % 4 == 0, "a round is whole passes of K1's 4-step loop");
// Rounds only in launches of at least this many steps per wave (256 Ki items
// on 256 CUs): the waves' first meeting costs 1-2 us that a short launch has
// no tail to win back.  Rounds of 4 steps: +2.5-4 % at 8 steps per wave,
// +1 % at 16, -1.7 % at 32, -3.5 % at 128 and 512 (same file).
constexpr uint32_t kK1RoundsMinSteps = 32;
// The barriers every wave of a K1 launch executes, whatever its own range: a
// function of cg alone (the steps of a full range, the same for every wave of
// the grid).  A wave arrives once per S steps it runs in its 4-step loop, as
// long as it owes an arrival (floor(nsteps / S) <= floor(cg / S) times), and
// makes up the rest after its last store (k_fixed.h).
MCRC_HD uint64_t k1_rounds(uint64_t cg, uint32_t S) { return cg >= kK1RoundsMinSteps ? cg / S : 0; }
// K1's order: which group (pair of items) a wave reads at which step of the
// static part.  W = nwg wv waves (nwg workgroups of wv waves), every wave cg
// steps: cg / 4 passes of K1's 4-step loop and a remainder of cg % 4 steps.
//   ranges (O0)       wave w = wv b + t streams the contiguous range r of cg
//                     groups, r = (w 65521) mod W: a bijection unless the prime
//                     divides W, and then the deal is left unscrambled
//   window by pass    workgroup b owns the wv cg contiguous groups of window rb
//   (O2)              (b dealt through the same scramble over nwg, or b itself);
//                     in pass q wave t reads the four groups
//                     base + 4 wv q + 4 t + j: 32 KiB contiguous per wave and
//                     pass, 32 wv KiB per workgroup and round.  The remainder:
//                     base + 4 wv (cg / 4) + (cg % 4) t + j
//   window by step    wave t reads base + wv s + t at step s: 8 wv KiB
//   (O1)              contiguous per workgroup and step
// The window orders run only in launches with lockstep rounds (cg >=
// kK1RoundsMinSteps): a window is read together only by waves that are paced
// together.  Shorter launches keep the ranges.
enum K1Order : uint32_t { kK1OrderRanges = 0, kK1OrderWindowStep = 1, kK1OrderWindowPass = 2 };
MCRC_HD uint64_t k1_scramble(uint64_t i, uint64_t n) { return n % 65521u ? (i * 65521u) % n : i; }
MCRC_HD K1Order k1_order_for(K1Order o, uint64_t cg) { return cg >= kK1RoundsMinSteps ? o : kK1OrderRanges; }
// One wave's walk: step j of pass q reads group first + q pstep + j sstep, step
// j of the remainder rfirst + j sstep; a group at or past end (or past the
// batch) is not the wave's and is not read.
struct K1Walk {
    uint64_t first, sstep, pstep, rfirst, end;
};
// (o: the order that runs, k1_order_for's; scramble: deal the windows through
// k1_scramble -- the ranges always are)
MCRC_HD K1Walk k1_walk(K1Order o, bool scramble, uint32_t b, uint32_t t, uint32_t nwg, uint32_t wv, uint64_t cg) {
    const uint64_t whole = cg & ~3ull, rem = cg & 3u;
    K1Walk k;
    if (o == kK1OrderRanges) {
        k.first = k1_scramble(b * wv + t, (uint64_t)nwg * wv) * cg;
        k.sstep = 1, k.pstep = 4;
        k.rfirst = k.first + whole;
        k.end = k.first + cg;
        return k;
    }
    const uint64_t base = (scramble ? k1_scramble(b, nwg) : b) * wv * cg;
    k.pstep = 4ull * wv;
    if (o == kK1OrderWindowPass) {
        k.first = base + 4ull * t;
        k.sstep = 1;
        k.rfirst = base + wv * whole + rem * t;
        k.end = k.rfirst + rem;  // (no remainder: the window's end)
    } else {
        k.first = base + t;
        k.sstep = wv;
        k.rfirst = base + wv * whole + t;
        k.end = base + wv * cg;
    }
    return k;
}
// The group that wave slot t of workgroup b reads at step j (0-3) of pass q
// (q = cg / 4: the remainder, j < cg % 4).
MCRC_HD uint64_t k1_group(K1Order o, bool scramble, uint32_t b, uint32_t t, uint64_t q, uint32_t j, uint32_t nwg,
                          uint32_t wv, uint64_t cg) {
    const K1Walk k = k1_walk(o, scramble, b, t, nwg, wv, cg);
    return (q < cg / 4 ? k.first + q * k.pstep : k.rfirst) + j * k.sstep;
}
// The order the product runs, and whether its windows are dealt scrambled.
// Libraries alternated with the parent's (the ranges) under bench.py on one
// box, ms per launch, medians (profiles/k1_order_ab.jsonl, four sessions; K1
// in every order in one process: profiles/k1_order_waves.txt):
//   items    ranges   window by pass     the same, scrambled   window by step (one process)
//   1 Mi     0.6267   0.6103 (-2.6 %)    level (0.6121 beside 0.6119)   -2.0 % (pass beside it -3.2 %)
//   4 Mi     2.5225   2.4402 (-3.3 %)    2.4417                -1.4 % (-2.2 %)
//   320 Ki   0.2045   0.2030 (-0.7 %)    0.2027                -1.3 % (-1.7 %)
// faster than the ranges in every round of every session (28 at 1 Mi items).
// The scramble buys nothing for windows, so they are dealt in launch order.
constexpr K1Order kK1Order = kK1OrderWindowPass;
constexpr bool kK1WindowScramble = false;
// K1's claimed tail: the XCDs do not run at one rate, so equal static shares
// leave the faster ones idle at the end of a launch.  The last 1 / 2^kK1TailShift
// of every range goes into a pool instead, cut into chunks of kK1TailSteps
// groups that the waves claim as they finish.  Chunk c belongs to sub-pool
// c % kK1TailPools (one per wave slot of a workgroup, a counter each), with
// index c / kK1TailPools in it.  The static part, groups [0, W cg_s), is K1's
// split of 2 W cg_s items: a full range of cg_s steps for every wave.
// Libraries alternated with the parent's on one box, ms per launch, medians
// (profiles/k1_tail_ab.jsonl; the parent's spread over the rounds 0.002 at 1 Mi
// items, 0.003-0.007 at 4 Mi):
//   items           parent   1/8, chunks of 4   1/16     1/4      chunks of 2
//   1 Mi            0.6373   0.6246 (-2.0 %)    +0.6 %   -0.3 %   0.6261 (-1.8 %)
//   4 Mi            2.5227   2.4646 (-2.3 %)                      2.4634 (-2.3 %, -2.6 % for 4 beside it)
// (1/16 and 1/4 in a session of their own: against the 1/8 library beside
// them +2.5 % and +1.6 %.  Chunks of 2: a variant that claims at the top of a
// chunk for the chunk after next and reads the claim at the chunk's bottom.)
constexpr uint32_t kK1TailShift = 3;
constexpr uint32_t kK1TailSteps = 4;  // (K1's 4-step pass: a chunk is one pass)
constexpr uint32_t kK1TailPools = 16;
// The smallest cg the split supports: from here on cg_s <= cg - 1, so the
// static part never reaches past the batch.
constexpr uint32_t kK1TailFloorSteps = 1u << kK1TailShift;
static_assert(kK1TailFloorSteps >= 8, "cg_s = 4 must leave a pool");
// The tail runs in launches of at least this many steps per wave (the default
// of crc32c_set_k1_tail_min; 320 Ki items on 256 CUs).  Against the parent,
// same file, the threshold set for the run: +10.5 % at 64 Ki items (8 steps per
// wave), +3.5 % at 128 Ki (16), +4.8 % at 256 Ki (32: a static part of 28 steps
// is also too short for the lockstep rounds); at 37 steps, the first static
// part of 32, -1.4 % in the median but not in every round; -3.4 % at 320 Ki
// (40), -2.1 % at 384 Ki (48), -1.5 % at 512 Ki (64), -2.0 % at 1 Mi (128),
// -2.3 % at 4 Mi (512).
constexpr uint32_t kK1TailMinSteps = 40;
static_assert(kK1TailMinSteps >= kK1RoundsMinSteps && kK1TailMinSteps >= kK1TailFloorSteps, "");
struct K1Tail {
    uint64_t cg_s;     // steps of every wave's static range (a multiple of 4, at least 4)
    uint64_t pool0;    // the pool's first group, W cg_s
    uint64_t nchunks;  // chunks of kK1TailSteps groups in [pool0, ngroups), the last one maybe cut
};
// (ngroups: pairs of items, the last maybe of one; W: the grid's waves; for
// ceil(ngroups / W) >= kK1TailFloorSteps)
MCRC_HD K1Tail k1_tail_split(uint64_t ngroups, uint64_t W) {
    const uint64_t cg = (ngroups + W - 1) / W;
    const uint64_t keep = (cg - (cg >> kK1TailShift)) & ~3ull;
    K1Tail t;
    t.cg_s = keep < 4 ? 4 : keep;
    t.pool0 = W * t.cg_s;
    t.nchunks = (ngroups - t.pool0 + kK1TailSteps - 1) / kK1TailSteps;
    return t;
}
// Chunks of sub-pool t: ceil((nchunks - t) / kK1TailPools), floored at 0.
MCRC_HD uint64_t k1_tail_pool_chunks(uint64_t nchunks, uint32_t t) {
    return nchunks > t ? (nchunks - t + kK1TailPools - 1) / kK1TailPools : 0;
}
// The counters of one stream's K1 launches (k1_slots.h): a claim head per
// sub-pool and the count of workgroups done, each on a 256-B line of its own
// (atomics on one line serialise like atomics on one word).  All zero between
// launches, kept so by the kernel's last workgroup.
struct K1Line {
    uint32_t v;
    uint32_t pad[63];
};
struct K1Ctl {
    K1Line head[kK1TailPools];
    K1Line done;
};
static_assert(sizeof(K1Line) == 256 && sizeof(K1Ctl) == 256 * (kK1TailPools + 1), "one line per counter");
constexpr uint32_t kRowBytes = 1024;  // a row: two of K1's 512-B piece rows (the head-block skip)
constexpr uint32_t kBlockBytes = 4 * kRowBytes;  // 4096
// (round 5: 128 KiB; config 3 -1.1..-1.3 % against 64 KiB in two sessions, the
// mixed pages and config 5 within noise, 256 KiB like 128 --
// profiles/r05_ablations/segment_size_ab.txt; rounds 1-3 found 24-64 KiB alike)
constexpr uint32_t kSegBytes = 128 * 1024;
// Longest span (CRC32C_MAX_SPAN): a unit's grid offsets (eo, G - p, the block
// count times 4 KiB) are 32-bit and signed, and a span that overlaps others
// past the plan's capacity is one unit.  Twice the largest item memcached
// stores (ITEM_SIZE_MAX_UPPER_LIMIT = 1 GiB, memcached.h:115).  Longer spans
// are not read (out = 0, counted as out of range / malformed).
constexpr uint32_t kMaxSpan = 0x7fff0000u;
// The planned path's grid (round 5): anchored at Ea = E rounded up to a
// 128-B line, so every block of a unit is whole lines and the span kernel's
// non-temporal loads never share a line between two instructions; the
// span's thread folds up to 127 foreign tail bytes instead of 15.
constexpr uint32_t kGridAlign = 128;
constexpr uint32_t kFragMax = 128;    // a head fragment [p, G1) of at most this
// (512 since round 5: 256-512 beat 1024 by 1.0-1.3 % on the mixed pages and
// matched it on config 3; 2048 / 3072 were 1-3 % slower --
// profiles/r05_ablations/whole_span_limit_ab.txt)
constexpr uint32_t kWholeMax = 512;   // a whole span of vlen at most this
// Is the head fragment (G1 - p = g1o) the span thread's?  For vlen <= kWholeMax
// the fragment is the whole span (G1 = Ea).
MCRC_HD bool frag_drop(uint32_t len, uint64_t g1o, uint64_t vlen) {
    return len != 0 && (g1o <= kFragMax || vlen <= kWholeMax);
}
constexpr uint32_t kLineBytes = 128;  // K5 (k_lines.h): an HBM line
constexpr uint32_t kEpoch = 32;       // K5: steps per epoch, 64 images per wave
// K5's fused shape: B - A (bytes of whole lines inside the span after the
// head) is 31 or 32 lines.
MCRC_HD bool lines_fused(int64_t lines_bytes) {
    return lines_bytes >= (int64_t)(kBlockBytes - kLineBytes) && lines_bytes <= (int64_t)kBlockBytes;
}
constexpr uint32_t kSmallMax = 8192;  // k_small: the spans of one launch at most
// The span kernel's workgroup: 16 waves per CU (128 VGPRs).  768 threads (168
// VGPRs) measured slower (config 3: 5.99 vs 5.90 ms; config 5: 6.90 vs 5.93 ms
// per 300 pages): the dependent lookup chains need the waves.
constexpr uint32_t kSpanBlock = 1024;
constexpr uint32_t kPlanThreads = 1024, kPlanPer = 2, kPlanTile = kPlanThreads * kPlanPer;  // k_plan.h: the scans
constexpr uint32_t kWalkWaves = 4;  // k_walk.h: waves (wbufs) per workgroup

}  // namespace mcrc_dev
