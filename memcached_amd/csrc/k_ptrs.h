// k_ptrs.h -- k_ptr_rebase: a device pointer batch (crc32c_batch_ptrs with
// CRC32C_DEVICE) turned into the offsets batch every span kernel takes.
#pragma once

#include "k_common.h"

namespace mcrc_dev {

constexpr uint32_t kPtrThreads = 256;

// v reduced over the wave's 64 lanes by OP, in every lane (64-bit values cross
// lanes as two dwords: __shfl_xor's own split).
template <class OP>
__device__ __forceinline__ unsigned long long wave_reduce64(unsigned long long v, OP op) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = op(v, (unsigned long long)__shfl_xor(v, m));
    return v;
}

// The spans of a pointer batch have no base and their lengths are on the
// device, so nothing on the host can size the plan or apply the small rule.
// Two launches of this kernel over ptrs[] and lens[] supply that:
//   emit == 0: red[0] = min(lo, the spans' starts), red[1] = max(hi, their
//     ends), red[2] += their lengths (red starts as {~0, 0, 0}).  A span of no
//     bytes is in none of them (its pointer may be NULL and must not drag lo to
//     0), nor is one longer than kMaxSpan (no kernel reads it).  A thread keeps
//     its three values in registers over a grid-stride loop, a wave folds them
//     with shuffles, a workgroup through LDS: three atomics per workgroup.
//   emit != 0, behind it on the stream: offsets[i] = ptrs[i] - red[0], so that
//     {base = lo, base_bytes = hi - lo, offsets} is the batch.  A span of no
//     bytes gets offset 0 (in range at any extent: out[i] = crc_in[i]); one
//     that is too long keeps whatever the subtraction gives and is refused by
//     its length.
__global__ __launch_bounds__(kPtrThreads) void k_ptr_rebase(const uint64_t *__restrict__ ptrs,
                                                            const uint32_t *__restrict__ lens, uint32_t len, uint64_t n,
                                                            unsigned long long *red, uint64_t *__restrict__ offsets,
                                                            uint32_t emit) {
    MCRC_VGPR_FLOOR();  // (several workgroups per CU: crc32c_device.h)
    const uint64_t i0 = blockIdx.x * (uint64_t)kPtrThreads + threadIdx.x, step = (uint64_t)gridDim.x * kPtrThreads;
    if (emit) {
        const uint64_t lo = red[0];
        for (uint64_t i = i0; i < n; i += step) offsets[i] = (lens ? lens[i] : len) ? ptrs[i] - lo : 0ull;
        return;
    }
    unsigned long long lo = ~0ull, hi = 0ull, sum = 0ull;
    for (uint64_t i = i0; i < n; i += step) {
        const uint32_t l = lens ? lens[i] : len;
        if (l != 0u && l <= kMaxSpan) {
            const unsigned long long p = ptrs[i];
            lo = p < lo ? p : lo;
            hi = p + l > hi ? p + l : hi;
            sum += l;
        }
    }
    lo = wave_reduce64(lo, [](unsigned long long x, unsigned long long y) { return x < y ? x : y; });
    hi = wave_reduce64(hi, [](unsigned long long x, unsigned long long y) { return x > y ? x : y; });
    sum = wave_reduce64(sum, [](unsigned long long x, unsigned long long y) { return x + y; });
    constexpr uint32_t kWaves = kPtrThreads / 64;
    __shared__ unsigned long long part[3][kWaves];
    if (__lane_id() == 0) {
        const uint32_t w = threadIdx.x / 64;
        part[0][w] = lo;
        part[1][w] = hi;
        part[2][w] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kWaves; ++w) {
            lo = part[0][w] < lo ? part[0][w] : lo;
            hi = part[1][w] > hi ? part[1][w] : hi;
            sum += part[2][w];
        }
        if (sum) {  // (a workgroup without a counted span has nothing to add)
            atomicMin(&red[0], lo);
            atomicMax(&red[1], hi);
            atomicAdd(&red[2], sum);
        }
    }
}

}  // namespace mcrc_dev
