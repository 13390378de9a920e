// repair_bytes_check.cpp -- the arithmetic of crc32c_repair_bytes
// (memcached_amd/csrc/repair_geom.h) and crc32c_locate_byte's source
// (memcached_amd/csrc/crc32c_host.cpp) run on the CPU.  The span limit is
// derived here, not believed: the smallest distance d at which two one-byte
// error patterns share a syndrome, B = B' x^(8 d) mod P, is recomputed from
// scratch over all 255 patterns.
//
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I memcached_amd/csrc repair_bytes_check.cpp
//       memcached_amd/csrc/crc32c_host.cpp
//
//   repair_bytes_check           every check; prints "repair_bytes ok"
//   repair_bytes_check locate    stdin: "crc_computed crc_stored len" per line,
//                                stdout: crc32c_locate_byte's "p mask" per line
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "../../include/crc32c_batch.h"
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

static uint32_t fwd8[256];  // g x^8 = (g >> 8) ^ fwd8[g & 0xff]
static uint32_t step8(uint32_t g) { return (g >> 8) ^ fwd8[g & 0xffu]; }

int main(int argc, char **argv) {
    if (argc > 1) {  // locate: the scalar over the caller's cases
        unsigned long long c, e, len;
        while (scanf("%llu %llu %llu", &c, &e, &len) == 3) {
            uint8_t m = 0x77;
            const uint64_t p = crc32c_locate_byte((uint32_t)c, (uint32_t)e, len, &m);
            printf("%llu %u\n", (unsigned long long)p, (unsigned)m);
        }
        return 0;
    }
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t g = b;
        for (int i = 0; i < 8; ++i) g = repair_step(g);
        fwd8[b] = g;
    }
    // (the table form of the forward byte step against eight bit steps, and against the search's step back)
    for (uint32_t i = 0, g = 0x12345678u; i < 100000; ++i, g = g * 1664525u + 1013904223u) {
        uint32_t f = g;
        for (int k = 0; k < 8; ++k) f = repair_step(f);
        CHECK(step8(g) == f && repair_unstep8(f) == g);
    }

    // The bound.  From each of the 255 patterns B' (a register confined to its top byte), d forward byte
    // steps: the first d at which any of them is confined to the top byte again is the smallest codeword
    // length at which one damaged byte could be taken for another.
    uint64_t best = ~0ull;
    uint32_t best_from = 0, best_to = 0;
    const uint64_t limit = (uint64_t)kRepairBytesSpanMax + 4;
    for (uint32_t b = 1; b < 256; ++b) {
        uint32_t g = b << 24;
        for (uint64_t d = 1; d <= limit && d < best; ++d) {
            g = step8(g);
            if (repair_byte_hit(g)) {
                best = d;
                best_from = b;
                best_to = repair_byte_mask(g);
            }
        }
    }
    CHECK(best == 190235);
    CHECK(best_from == 0xdf && best_to == 0x4c);
    CHECK((uint64_t)kRepairBytesSpanMax + 4 == best);
    CHECK(kRepairBytesSpanMax == CRC32C_REPAIR_BYTES_SPAN_MAX && kRepairBytesSpanDefault == CRC32C_REPAIR_BYTES_SPAN_DEFAULT);
    CHECK((((uint64_t)kRepairBytesSpanMax + 4) << 8) < kRepairNone);  // (a step and a mask in one 32-bit word)

    // the hit test: non-zero and nothing below the top byte
    CHECK(!repair_byte_hit(0) && !repair_byte_hit(0x00800000u) && !repair_byte_hit(0x80000001u) &&
          !repair_byte_hit(0xff000100u));
    for (uint32_t m = 1; m < 256; ++m) {
        CHECK(repair_byte_hit(m << 24) && repair_byte_mask(m << 24) == m);
        CHECK(repair_hit(m << 24) == ((m & (m - 1)) == 0));  // (the one-bit hits are among them)
    }

    // step <-> byte against the one-bit geometry: bit b of codeword byte p has t = 8 j + r with j the
    // byte's step and x^r the register bit that is bit b of the mask
    for (uint64_t len : {0ull, 1ull, 2ull, 20ull, 251ull, 252ull, 253ull, 4133ull, (unsigned long long)kRepairBytesSpanMax}) {
        for (uint64_t p = 0; p < 4 + len; ++p) {
            if (len > 5000 && p > 600 && p + 600 < 4 + len && p % 977) continue;
            const uint64_t j = repair_step_of_byte(p, len);
            CHECK(j < repair_steps(len) && repair_byte_of_step(j, len) == p);
            for (uint32_t b = 0; b < 8; ++b) {
                const uint64_t t = repair_t_of_q(8 * p + b, len);
                CHECK(t / 8 == j);
                const uint32_t v = kRepairOne >> (t % 8);
                CHECK(repair_byte_hit(v) && repair_byte_mask(v) == (1u << b));
            }
        }
        CHECK(repair_byte_of_step(0, len) == 3 && repair_byte_of_step(3, len) == 0);
        if (len) CHECK(repair_byte_of_step(4, len) == 4 + len - 1 && repair_byte_of_step(4 + len - 1, len) == 4);
    }

    // the length bits of a (byte, mask) pair: repair_length_bit of any bit the mask inverts
    for (uint64_t by = 0; by < 64; ++by)
        for (uint32_t m = 1; m < 256; ++m) {
            bool want = false;
            for (uint32_t b = 0; b < 8; ++b)
                if (m >> b & 1) want = want || repair_length_bit(8 * by + b);
            CHECK(repair_length_mask(by, m) == want);
        }

    // crc32c_locate_byte: S = (m << 24) x^(8 j) stepped forward, every step of short spans and the steps
    // around the chunk edge and the end of long ones, masks of every weight
    const uint32_t masks[] = {0x01, 0x80, 0x03, 0xff, 0x5a, 0xdf, 0x4c};
    for (uint64_t len : {0ull, 1ull, 20ull, 251ull, 252ull, 253ull, 4133ull, (unsigned long long)kRepairBytesSpanMax}) {
        for (uint32_t m : masks) {
            uint32_t g = m << 24;
            for (uint64_t j = 0; j < repair_steps(len); ++j, g = step8(g)) {
                if (len > 300 && j > 8 && (j < 250 || j > 262) && j + 3 < repair_steps(len)) continue;
                uint8_t got = 0x77;
                const uint32_t e = (uint32_t)(j * 2654435761u) ^ m;
                CHECK(crc32c_locate_byte(g ^ e, e, len, &got) == repair_byte_of_step(j, len) && got == m);
                if ((m & (m - 1)) == 0) {  // a single bit: crc32c_locate_bit's position
                    uint32_t b = 0;
                    while (!(m >> b & 1)) ++b;
                    CHECK(crc32c_locate_bit(g ^ e, e, len) == 8 * repair_byte_of_step(j, len) + b);
                }
            }
            // the first byte behind the codeword (at the limit it is 0xdf's twin: see above)
            uint8_t got = 0x77;
            if (len < kRepairBytesSpanMax)
                CHECK(crc32c_locate_byte(g, 0, len, &got) == CRC32C_NO_BIT && got == 0);
        }
    }
    {
        uint8_t got = 0x77;
        CHECK(crc32c_locate_byte(5, 5, 100, &got) == CRC32C_NO_BIT && got == 0);
        got = 0x77;
        CHECK(crc32c_locate_byte(kRepairOne, 0, (uint64_t)kRepairBytesSpanMax + 1, &got) == CRC32C_NO_BIT && got == 0);
        CHECK(crc32c_locate_byte(kRepairOne, 0, kRepairBytesSpanMax, &got) == 3 && got == 0x80);
        CHECK(crc32c_locate_byte(0x03000000u, 0, 0, nullptr) == 3);  // (the mask is optional)
        // damage in two bytes: 0x00010100 is no single byte's pattern in a 20-byte span
        CHECK(crc32c_locate_byte(0x00010100u, 0, 20, &got) == CRC32C_NO_BIT);
    }
    if (fails) return 1;
    printf("repair_bytes ok\n");
    return 0;
}
