// k1_order_check.cpp -- K1's order (k1_walk / k1_group, k_consts.h) checked on
// the CPU: plain C++ over the header the kernel compiles, built with
// -fsanitize=address,undefined by tests/test_k1_order_model.py.
//
//   k1_order_check ORDER SCRAMBLE NWG WV CG [ORDER SCRAMBLE NWG WV CG ...]
//
// Per case one line:
//   RUN ROUNDS SUM PERM LAYOUT
// RUN     the order that runs at CG steps per wave (k1_order_for)
// ROUNDS  k1_rounds(CG, kK1RoundSteps), the barriers every wave owes
// SUM     sum over (b, t, s) in that order of group x (index + 1), mod 2^64,
//         s = 4 q + j over the passes and the remainder: the whole mapping, to
//         be compared with the Python restatement's
// PERM    1 if the groups below each wave's end are a permutation of
//         [0, NWG WV CG): none read twice, none missed
// LAYOUT  1 if every pass has the order's stated shape
// Exit status 1 if any PERM or LAYOUT is 0.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "k_consts.h"

using namespace mcrc_dev;

static bool layout_ok(K1Order run, bool scr, uint32_t nwg, uint32_t wv, uint64_t cg) {
    const uint64_t Q = cg / 4, rem = cg % 4;
    for (uint32_t b = 0; b < nwg; ++b) {
        const uint64_t rb = run == kK1OrderRanges || !scr ? b : k1_scramble(b, nwg);
        const uint64_t base = rb * wv * cg;
        for (uint32_t t = 0; t < wv; ++t) {
            const K1Walk k = k1_walk(run, scr, b, t, nwg, wv, cg);
            for (uint64_t q = 0; q <= Q; ++q)
                for (uint32_t j = 0; j < (q < Q ? 4u : (uint32_t)rem); ++j) {
                    const uint64_t g = k1_group(run, scr, b, t, q, j, nwg, wv, cg);
                    uint64_t want;
                    if (run == kK1OrderRanges)  // the wave's range, in sequence
                        want = k1_scramble((uint64_t)b * wv + t, (uint64_t)nwg * wv) * cg + 4 * q + j;
                    else if (run == kK1OrderWindowPass)  // four neighbours; 4 wv per workgroup and pass
                        want = q < Q ? base + 4ull * wv * q + 4 * t + j : base + 4ull * wv * Q + rem * t + j;
                    else  // wv neighbours per workgroup and step
                        want = base + (uint64_t)wv * (4 * q + j) + t;
                    if (g != want || g >= k.end) return false;
                }
        }
    }
    return true;
}

int main(int argc, char **argv) {
    int bad = 0;
    for (int i = 1; i + 4 < argc; i += 5) {
        const K1Order o = (K1Order)atoi(argv[i]);
        const bool scr = atoi(argv[i + 1]) != 0;
        const uint32_t nwg = (uint32_t)strtoul(argv[i + 2], nullptr, 10), wv = (uint32_t)strtoul(argv[i + 3], nullptr, 10);
        const uint64_t cg = strtoull(argv[i + 4], nullptr, 10);
        const K1Order run = k1_order_for(o, cg);
        const uint64_t total = (uint64_t)nwg * wv * cg, Q = cg / 4, rem = cg % 4;
        std::vector<unsigned char> seen(total, 0);
        uint64_t sum = 0, idx = 0;
        bool perm = true;
        for (uint32_t b = 0; b < nwg; ++b)
            for (uint32_t t = 0; t < wv; ++t)
                for (uint64_t q = 0; q <= Q; ++q)
                    for (uint32_t j = 0; j < (q < Q ? 4u : (uint32_t)rem); ++j) {
                        const uint64_t g = k1_group(run, scr, b, t, q, j, nwg, wv, cg);
                        sum += g * ++idx;
                        if (g >= total || seen[g]) perm = false;
                        else seen[g] = 1;
                    }
        perm = perm && idx == total;
        const bool lay = layout_ok(run, scr, nwg, wv, cg);
        bad += !perm || !lay;
        printf("%u %llu %llu %d %d\n", (unsigned)run, (unsigned long long)k1_rounds(cg, kK1RoundSteps),
               (unsigned long long)sum, (int)perm, (int)lay);
    }
    return bad ? 1 : 0;
}
