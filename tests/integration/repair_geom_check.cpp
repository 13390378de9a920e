// repair_geom_check.cpp -- the arithmetic of crc32c_repair_items
// (memcached_amd/csrc/repair_geom.h) and crc32c_locate_bit's source
// (memcached_amd/csrc/crc32c_host.cpp) run on the CPU, against bit-by-bit
// stepping of the syndrome sequence g(t).
//
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I memcached_amd/csrc repair_geom_check.cpp
//       memcached_amd/csrc/crc32c_host.cpp
//
//   repair_geom_check           every check; prints "repair_geom ok"
//   repair_geom_check locate    stdin: "crc_computed crc_stored len" per line,
//                               stdout: crc32c_locate_bit's answer per line
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/crc32c_batch.h"
#include "crc32c_gf2.h"
#include "repair_geom.h"

using namespace mcrc;

static int fails = 0;
#define CHECK(c)                                             \
    do {                                                     \
        if (!(c)) {                                          \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                         \
        }                                                    \
    } while (0)

static uint32_t rnd(uint64_t *s) {
    *s = *s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(*s >> 32);
}

int main(int argc, char **argv) {
    if (argc > 1) {  // locate: the scalar over the caller's cases
        unsigned long long c, e, len;
        while (scanf("%llu %llu %llu", &c, &e, &len) == 3)
            printf("%llu\n", (unsigned long long)crc32c_locate_bit((uint32_t)c, (uint32_t)e, len));
        return 0;
    }
    uint64_t seed = 7;
    // the step and its inverse, the byte step and its table form
    uint32_t inv8[256];
    for (uint32_t b = 0; b < 256; ++b) inv8[b] = repair_unstep8(b << 24);
    for (int i = 0; i < 100000; ++i) {
        const uint32_t g = rnd(&seed);
        CHECK(repair_unstep(repair_step(g)) == g && repair_step(repair_unstep(g)) == g);
        CHECK(repair_step(g) == mulmodp(g, 0x40000000u));
        uint32_t f = g;
        for (int k = 0; k < 8; ++k) f = repair_step(f);
        CHECK(repair_unstep8(f) == g);
        CHECK(((g << 8) ^ inv8[g >> 24]) == repair_unstep8(g));
    }
    // x^(2^31 - 1) = 1 (2^31 - 1 is prime and x != 1: that is x's order), and the span limit stays below it
    {
        uint32_t r = kRepairOne, sq = 0x40000000u;
        for (uint64_t e = kRepairOrder; e; e >>= 1) {
            if (e & 1) r = mulmodp(r, sq);
            sq = mulmodp(sq, sq);
        }
        CHECK(r == kRepairOne);
        CHECK(32 + 8 * (uint64_t)kRepairSpanMax < kRepairOrder);
        CHECK(32 + 8 * ((uint64_t)kRepairSpanMax + 64) >= kRepairOrder);
    }
    // positions: q <-> t round trips, t covers [0, 32 + 8 L) once, the ends
    for (uint64_t len : {1ull, 2ull, 20ull, 255ull, 256ull, 257ull, 4133ull}) {
        const uint64_t np = repair_positions(len);
        std::vector<uint8_t> seen(np, 0);
        for (uint64_t q = 0; q < np; ++q) {
            const uint64_t t = repair_t_of_q(q, len);
            CHECK(t < np && !seen[t]);
            if (t < np) seen[t] = 1;
            CHECK(repair_q_of_t(t, len) == q);
        }
        CHECK(repair_t_of_q(0, len) == 31 && repair_t_of_q(31, len) == 0);
        CHECK(repair_t_of_q(32 + 8 * (len - 1) + 7, len) == 32 && repair_t_of_q(32, len) == np - 1);
        CHECK(repair_steps(len) * 8 == np);
        CHECK(repair_nchunks(len) == (len + 4 + kRepairChunk - 1) / kRepairChunk);
    }
    // hits: exactly the eight single bits of the top byte
    for (uint32_t r = 0; r < 32; ++r) {
        const uint32_t v = kRepairOne >> r;
        CHECK(repair_hit(v) == (r < 8));
        if (r < 8) CHECK(repair_hit_r(v) == r);
    }
    CHECK(!repair_hit(0) && !repair_hit(0xc0000000u) && !repair_hit(0x80000001u) && !repair_hit(0x00800000u));
    // chunk starts: S x^(-8 j0) by the power table's exponent, against byte steps from S
    for (int rep = 0; rep < 8; ++rep) {
        const uint32_t S = rnd(&seed) | 1u;
        uint32_t v = S;
        for (uint64_t j = 0; j <= 5 * kRepairChunk; ++j) {
            if (j % kRepairChunk == 0 || j == 1) {
                const uint64_t n = repair_chunk_pow(j);
                CHECK((j ? mulmodp(S, xpow8n(n)) : S) == v);
            }
            v = repair_unstep8(v);
        }
    }
    CHECK(mulmodp(xpow8n(repair_chunk_pow(1ull << 28)), xpow8n(1ull << 28)) == kRepairOne);
    // crc32c_locate_bit: every position of spans of 0..40 bytes and of the lengths around a chunk, S = g(t)
    // stepped bit by bit; every two-bit pattern of a 20-byte span and the other refusals: none
    for (uint64_t len : {0ull, 1ull, 2ull, 3ull, 20ull, 40ull, 251ull, 252ull, 253ull, 4133ull}) {
        uint32_t g = kRepairOne;
        for (uint64_t t = 0; t < repair_positions(len); ++t, g = repair_step(g)) {
            if (len > 300 && t % 97 && t + 40 < repair_positions(len)) continue;
            const uint32_t e = rnd(&seed);
            CHECK(crc32c_locate_bit(g ^ e, e, len) == repair_q_of_t(t, len));
        }
        // the first position behind the codeword
        CHECK(crc32c_locate_bit(g, 0, len) == CRC32C_NO_BIT);
    }
    {
        const uint64_t len = 20, np = repair_positions(len);
        std::vector<uint32_t> gs(np);
        uint32_t g = kRepairOne;
        for (uint64_t t = 0; t < np; ++t, g = repair_step(g)) gs[t] = g;
        for (uint64_t a = 0; a < np; ++a)
            for (uint64_t b = a + 1; b < np; ++b) CHECK(crc32c_locate_bit(gs[a] ^ gs[b], 0, len) == CRC32C_NO_BIT);
    }
    CHECK(crc32c_locate_bit(5, 5, 100) == CRC32C_NO_BIT);
    CHECK(crc32c_locate_bit(kRepairOne, 0, (uint64_t)CRC32C_REPAIR_SPAN_MAX + 1) == CRC32C_NO_BIT);
    CHECK(crc32c_locate_bit(kRepairOne, 0, 0) == 31 && crc32c_locate_bit(1, 0, 0) == 0);
    // the length bits
    for (uint64_t k = 0; k < 8 * 64; ++k) {
        const uint64_t by = k / 8, b = k % 8;
        const bool want = (by >= 32 && by < 36) || by == 41 || (by == 38 && b == 1) || (by == 39 && b == 0);
        CHECK(repair_length_bit(k) == want);
    }
    if (fails) return 1;
    printf("repair_geom ok\n");
    return 0;
}
