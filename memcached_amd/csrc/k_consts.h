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
