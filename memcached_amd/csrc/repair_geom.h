// repair_geom.h -- the arithmetic of crc32c_repair_items that needs no GPU: the
// positions of an image's stored CRC and span, the exponent t each one has in
// the syndrome, the one-bit step and its inverse, the byte step the search
// takes, the chunks it is cut into and the header bits that decide an image's
// length, and at the end crc32c_repair_bytes' byte hit test and maps.  Plain
// C++ over k_consts.h (k_repair.h, k_repair_bytes.h, shim_repair.h,
// crc32c_locate_bit and crc32c_locate_byte use it;
// tests/integration/repair_geom_check.cpp and repair_bytes_check.cpp run it on
// the CPU).
//
// The rule (include/crc32c_batch.h).  A register holds a polynomial mod P
// reflected: bit 31 is x^0, so 0x80000000 is 1 and g -> (g >> 1) ^ (g & 1 ? P : 0)
// multiplies by x.  With c the CRC computed over a span of L bytes, e the
// stored one and S = c ^ e, inverting one bit of the codeword (the stored CRC
// followed by the span) makes S = x^t, where t counts the bit's distance from
// the codeword's end in the order the CRC shifts bits: stored-CRC bit j has
// t = 31 - j, bit b of span byte m has t = 32 + 8 (L - 1 - m) + (7 - b).  x has
// order 2^31 - 1 mod P, so below that many positions t is unique.
#pragma once

#include <stdint.h>

#include "k_consts.h"

namespace mcrc {

constexpr uint32_t kRepairPoly = 0x82f63b78u;       // P, reflected (crc32c.c:50)
constexpr uint32_t kRepairOne = 0x80000000u;        // x^0
constexpr uint32_t kRepairSpanMax = 0x0fffffc0u;    // CRC32C_REPAIR_SPAN_MAX: 32 + 8 L < 2^31 - 1
constexpr uint32_t kRepairSpanDefault = 2u << 20;   // CRC32C_REPAIR_SPAN_DEFAULT
constexpr uint64_t kRepairNoBit = ~0ull;            // CRC32C_NO_BIT
constexpr uint32_t kRepairNone = 0xffffffffu;       // the search's "no t" (t < 2^31)
constexpr uint64_t kRepairOrder = 0x7fffffffull;    // the order of x mod P
// The search goes through the positions a byte (8 values of t) at a time, in
// chunks of kRepairChunk byte steps: one lane per chunk.
constexpr uint32_t kRepairChunk = 256;

// g x and g x^-1.
MCRC_HD uint32_t repair_step(uint32_t g) { return (g >> 1) ^ ((g & 1u) ? kRepairPoly : 0u); }
MCRC_HD uint32_t repair_unstep(uint32_t g) {
    // (P has bit 31 set and g >> 1 never has: bit 31 says whether P was added)
    return (g & kRepairOne) ? ((g ^ kRepairPoly) << 1) | 1u : g << 1;
}
// g x^-8 bit by bit; the byte table of the search is repair_unstep8(b << 24),
// and g x^-8 = (g << 8) ^ table[g >> 24] (the step is linear and the low 24
// bits only move up).
MCRC_HD uint32_t repair_unstep8(uint32_t g) {
    for (int i = 0; i < 8; ++i) g = repair_unstep(g);
    return g;
}

// Positions from the stored CRC's first bit: q < 32 is bit q of the stored CRC
// (little-endian dword, LSB = 0), q >= 32 bit (q - 32) % 8 of span byte
// (q - 32) / 8.  For an item image k = 224 + q.
MCRC_HD uint64_t repair_positions(uint64_t len) { return 32 + 8 * len; }
MCRC_HD uint64_t repair_t_of_q(uint64_t q, uint64_t len) {
    if (q < 32) return 31 - q;
    const uint64_t m = (q - 32) / 8, b = (q - 32) % 8;
    return 32 + 8 * (len - 1 - m) + (7 - b);
}
MCRC_HD uint64_t repair_q_of_t(uint64_t t, uint64_t len) {
    if (t < 32) return 31 - t;
    const uint64_t u = t - 32;
    return 32 + 8 * (len - 1 - u / 8) + (7 - u % 8);
}

// The search.  V_j = S x^(-8 j), j = 0 .. steps - 1 (steps = 4 + L: every byte
// of the codeword).  S = x^t with t = 8 j + r, r < 8, exactly when V_j = x^r: a
// single bit inside the register's top byte, r = its distance from bit 31.
MCRC_HD uint64_t repair_steps(uint64_t len) { return 4 + len; }
MCRC_HD uint64_t repair_nchunks(uint64_t len) { return (repair_steps(len) + kRepairChunk - 1) / kRepairChunk; }
MCRC_HD bool repair_hit(uint32_t v) { return v >= 0x01000000u && (v & (v - 1u)) == 0u; }
MCRC_HD uint32_t repair_hit_r(uint32_t v) {  // (v: a hit)
    uint32_t r = 0;
    while (!((v << r) & kRepairOne)) ++r;
    return r;
}
// A chunk's first value is S x^(-8 j0); x^(-8 j0) = x^(8 n) with n =
// (2^31 - 1) - j0 for 0 < j0 < 2^31 - 1, which the power table (x^(8 n), n <
// 2^33) holds.  0: no multiply.
MCRC_HD uint64_t repair_chunk_pow(uint64_t j0) { return j0 ? kRepairOrder - j0 : 0; }

// The header bits that decide ITEM_ntotal, by the image's bit index k: nbytes
// (bytes 32..35), nkey (byte 41), it_flags bit 1 (ITEM_CAS: byte 38 bit 1) and
// bit 8 (ITEM_CFLAGS: byte 39 bit 0).  An image with one of them inverted
// would not verify over its own span.
MCRC_HD bool repair_length_bit(uint64_t k) {
    const uint64_t byte = k / 8, b = k % 8;
    return (byte >= 32 && byte <= 35) || byte == 41 || (byte == 38 && b == 1) || (byte == 39 && b == 0);
}

// crc32c_repair_bytes: the same search with another hit test.  V_j = S x^(-8 j)
// is non-zero and confined to the register's top byte exactly when the error
// pattern V_j lies in the codeword byte that step j covers, whatever its
// weight; bit 31 - r of V_j is that byte's bit 7 - r (repair_q_of_t of t =
// 8 j + r), so V_j >> 24 is the byte's XOR mask as it stands.  Two one-byte
// patterns d bytes apart share a syndrome iff B = B' x^(8 d) mod P; the smallest
// such d over all 255 patterns is 190 235 (0xdf against 0x4c;
// tests/integration/repair_bytes_check.cpp recomputes it), so a codeword of
// 4 + L <= 190 235 bytes has its damaged byte located at one place only.
constexpr uint32_t kRepairBytesSpanMax = 190231u;       // CRC32C_REPAIR_BYTES_SPAN_MAX: 4 + L <= 190 235
constexpr uint32_t kRepairBytesSpanDefault = 0x10000u;  // CRC32C_REPAIR_BYTES_SPAN_DEFAULT
MCRC_HD bool repair_byte_hit(uint32_t v) { return v != 0u && !(v & 0x00ffffffu); }
MCRC_HD uint32_t repair_byte_mask(uint32_t v) { return v >> 24; }  // (v: a byte hit)
// Codeword bytes: p < 4 is stored-CRC byte p, p >= 4 span byte p - 4 (image byte
// 28 + p).  Step j < 4 covers stored-CRC byte 3 - j, step j >= 4 span byte
// L + 3 - j; the map is its own inverse.
MCRC_HD uint64_t repair_byte_of_step(uint64_t j, uint64_t len) { return j < 4 ? 3 - j : len + 7 - j; }
MCRC_HD uint64_t repair_step_of_byte(uint64_t p, uint64_t len) { return p < 4 ? 3 - p : len + 7 - p; }
// repair_length_bit for each bit that mask m inverts in image byte `byte`.
MCRC_HD bool repair_length_mask(uint64_t byte, uint32_t m) {
    return (byte >= 32 && byte <= 35) || byte == 41 || (byte == 38 && (m & 0x02u)) || (byte == 39 && (m & 0x01u));
}

}  // namespace mcrc
