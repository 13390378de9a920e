// k_window.h -- a whole 4 KiB window in K1's lane layout (k_common.h), as K4
// (k_blocks) and K5 (k_lines) hold it.  K1 itself works on half items
// (K1Half, k_fixed.h).
#pragma once

#include "k_common.h"

namespace mcrc_dev {

struct K1Regs {
    uint4 d[kK1Pieces];  // piece k: item bytes [512 k + 16 i, +16) for lane i
    uint32_t cin;        // the item's initial CRC
    // wb: wave-uniform base (SGPR), loff: this lane's offset from it
    // Non-temporal: the windows are whole lines (128-B aligned); a 16-B
    // anchored block shares its end lines with its neighbours, which a
    // non-temporal load fetches twice
    __device__ __forceinline__ void load_at(const uint8_t *__restrict__ wb, uint32_t loff) {
#pragma unroll
        for (int k = 0; k < (int)kK1Pieces; ++k) d[k] = ld16_nt(wb + loff + k * kK1Piece);
    }
};

// The lane value M_{2048}(u_A) ^ u_B: u_A / u_B the first / second half's
// four chains, each ended by its shifted last step.
__device__ __forceinline__ uint32_t k1_lane_value(const K1Regs &r, const LaneCtx &c) {
    constexpr uint32_t kShift[3] = {kAuxShift0, kAuxShift1, kAuxShift2};  // M_1536, M_1024, M_512
    uint32_t x[kK1Pieces];
#pragma unroll
    for (int k = 0; k < (int)kK1Pieces; ++k) x[k] = r.d[k].x;
#pragma unroll
    for (int i = 1; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < (int)kK1Pieces; ++k) x[k] = step4_next(x[k], dw4(r.d[k], i), c);
#pragma unroll
    for (int k = 0; k < (int)kK1Pieces; ++k)
        x[k] = (k & 3) < 3 ? step4_last_shifted(x[k], kShift[k & 3]) : step4_next(x[k], 0u, c);
    const uint32_t ua = xor3(x[0], x[1], x[2]) ^ x[3], ub = xor3(x[4], x[5], x[6]) ^ x[7];
    return apply_op<4>(kAuxSpanFold, ua) ^ ub;
}

}  // namespace mcrc_dev
